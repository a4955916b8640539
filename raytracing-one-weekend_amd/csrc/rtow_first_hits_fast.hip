// Fast arithmetic build of the first-k-hits query kernel (rtow_first_hits.h): -ffp-contract=fast, the fast build's walks.
#define RTOW_SUFFIX fast
#define RTOW_FAST_MATH 1
#include "rtow_first_hits.h"
