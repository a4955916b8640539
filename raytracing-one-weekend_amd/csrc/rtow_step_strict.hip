// Strict arithmetic build of the path-step query kernel (rtow_step.h): -ffp-contract=off, bit-identical to the oracle's next segment.
#define RTOW_SUFFIX strict
#include "rtow_step.h"
