// Strict arithmetic build of the occlusion query kernel (rtow_occlude.h): -ffp-contract=off, the oracle's hit tests.
#define RTOW_SUFFIX strict
#include "rtow_occlude.h"
