// Strict arithmetic build of the ambient query kernel (rtow_ambient.h): -ffp-contract=off, the oracle's hit tests.
#define RTOW_SUFFIX strict
#include "rtow_ambient.h"
