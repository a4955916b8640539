// Fast arithmetic build of the camera-ray and guide-buffer kernels (rtow_guides.h): -ffp-contract=fast, the fast build's walks.
#define RTOW_SUFFIX fast
#define RTOW_FAST_MATH 1
#include "rtow_guides.h"
