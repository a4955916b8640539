// Strict arithmetic build of the closest-point query kernel (rtow_pointq.h): -ffp-contract=off, the formulas as written.
#define RTOW_SUFFIX strict
#include "rtow_pointq.h"
