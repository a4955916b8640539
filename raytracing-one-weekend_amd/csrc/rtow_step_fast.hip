// Fast arithmetic build of the path-step query kernel (rtow_step.h): -ffp-contract=fast, the fast build's walks.
#define RTOW_SUFFIX fast
#define RTOW_FAST_MATH 1
#include "rtow_step.h"
