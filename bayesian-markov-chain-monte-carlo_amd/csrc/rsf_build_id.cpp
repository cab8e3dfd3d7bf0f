// rsf_build_id.cpp — rsf_build_id(): what profiler evidence stored under profiles/ is keyed by.  The one unit that sees
// RSF_BUILD_ID, so that a change to any source recompiles nothing else on its account (csrc/Makefile).
#include "../../include/rsf_abi.h"

#ifndef RSF_BUILD_ID  // csrc/Makefile passes the SHA-256 prefix of the units' sources and headers
#define RSF_BUILD_ID "unknown"
#endif

extern "C" const char *rsf_build_id(void) { return RSF_BUILD_ID; }
