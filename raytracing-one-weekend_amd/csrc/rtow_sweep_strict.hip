// Strict arithmetic build of the swept-sphere query kernel (rtow_sweep.h): -ffp-contract=off, the formulas as written.
#define RTOW_SUFFIX strict
#include "rtow_sweep.h"
