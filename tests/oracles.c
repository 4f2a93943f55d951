/*
 * oracles.c -- the one translation unit of tests/libtest_oracles.so (tests/oracles.py builds it).  TEST INFRASTRUCTURE.
 * camera_oracle.c includes oracle/pt_oracle.c whole; each of the others builds on its statics and on those of the files before it.
 */
#include "camera_oracle.c"
#include "query_oracle.c"
#include "ao_oracle.c"
#include "direct_oracle.c"
#include "indirect_oracle.c"
#include "mis_oracle.c"
#include "primary_accept.c"
#include "extent_oracle.c"
