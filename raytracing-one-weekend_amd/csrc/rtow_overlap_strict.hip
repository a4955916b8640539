// Strict arithmetic build of the box-overlap query kernel (rtow_overlap.h): -ffp-contract=off, the predicates as written.
#define RTOW_SUFFIX strict
#include "rtow_overlap.h"
