// Fast arithmetic build of the swept-sphere query kernel (rtow_sweep.h): -ffp-contract=fast, refined hardware seeds.
#define RTOW_SUFFIX fast
#define RTOW_FAST_MATH 1
#include "rtow_sweep.h"
