// Strict arithmetic build of the first-k-hits query kernel (rtow_first_hits.h): -ffp-contract=off, the oracle's hit tests.
#define RTOW_SUFFIX strict
#include "rtow_first_hits.h"
