// Fast arithmetic build of the k-nearest query kernel (rtow_nearest.h): -ffp-contract=fast, refined hardware seeds.
#define RTOW_SUFFIX fast
#define RTOW_FAST_MATH 1
#include "rtow_nearest.h"
