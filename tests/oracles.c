/*
 * oracles.c -- the one translation unit of tests/libtest_oracles.so (tests/oracles.py builds it).  TEST INFRASTRUCTURE.
 * camera_oracle.c includes oracle/pt_oracle.c whole; the other two build on its statics and on camera_oracle.c's.
 */
#include "camera_oracle.c"
#include "query_oracle.c"
#include "ao_oracle.c"
