/*
 * direct_oracles.c -- the one translation unit of tests/libtest_direct_oracle.so (tests/direct_oracle.py builds it).
 * TEST INFRASTRUCTURE.  oracles.c brings oracle/pt_oracle.c and the camera, query and AO restatements whole; direct_oracle.c
 * builds on their statics.
 */
#include "oracles.c"
#include "direct_oracle.c"
