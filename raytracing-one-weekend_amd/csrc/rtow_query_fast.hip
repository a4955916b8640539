// Fast arithmetic build of the ray query kernel (rtow_query.h): -ffp-contract=fast, the fast build's walks.
#define RTOW_SUFFIX fast
#define RTOW_FAST_MATH 1
#include "rtow_query.h"
