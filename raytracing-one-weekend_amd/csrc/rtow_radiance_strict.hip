// Strict arithmetic build of the radiance query kernel (rtow_radiance.h): -ffp-contract=off, bit-identical to the oracle's ray_color.
#define RTOW_SUFFIX strict
#include "rtow_radiance.h"
