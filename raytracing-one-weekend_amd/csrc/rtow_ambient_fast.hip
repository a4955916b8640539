// Fast arithmetic build of the ambient query kernel (rtow_ambient.h): -ffp-contract=fast, the fast build's walks.
#define RTOW_SUFFIX fast
#define RTOW_FAST_MATH 1
#include "rtow_ambient.h"
