// Strict arithmetic build of the k-nearest query kernel (rtow_nearest.h): -ffp-contract=off, the formulas as written.
#define RTOW_SUFFIX strict
#include "rtow_nearest.h"
