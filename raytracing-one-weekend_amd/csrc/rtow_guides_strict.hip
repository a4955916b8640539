// Strict arithmetic build of the camera-ray and guide-buffer kernels (rtow_guides.h): -ffp-contract=off, bit-identical to the oracle's primaries.
#define RTOW_SUFFIX strict
#include "rtow_guides.h"
