// Fast arithmetic build of the box-overlap query kernel (rtow_overlap.h): -ffp-contract=fast.
#define RTOW_SUFFIX fast
#define RTOW_FAST_MATH 1
#include "rtow_overlap.h"
