// Fast arithmetic build of the radiance query kernel (rtow_radiance.h): -ffp-contract=fast, the fast build's walks.
#define RTOW_SUFFIX fast
#define RTOW_FAST_MATH 1
#include "rtow_radiance.h"
