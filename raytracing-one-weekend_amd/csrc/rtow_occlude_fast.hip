// Fast arithmetic build of the occlusion query kernel (rtow_occlude.h): -ffp-contract=fast, the fast build's walks.
#define RTOW_SUFFIX fast
#define RTOW_FAST_MATH 1
#include "rtow_occlude.h"
