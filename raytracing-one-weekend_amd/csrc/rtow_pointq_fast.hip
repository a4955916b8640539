// Fast arithmetic build of the closest-point query kernel (rtow_pointq.h): -ffp-contract=fast, refined hardware seeds.
#define RTOW_SUFFIX fast
#define RTOW_FAST_MATH 1
#include "rtow_pointq.h"
