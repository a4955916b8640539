// Strict arithmetic build of the ray query kernel (rtow_query.h): -ffp-contract=off, bit-identical to the oracle's hit tests.
#define RTOW_SUFFIX strict
#include "rtow_query.h"
