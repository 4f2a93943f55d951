/*
 * mis_oracles.c -- the one translation unit of tests/libtest_mis_oracle.so (tests/mis_oracle.py builds it).  TEST INFRASTRUCTURE.
 * indirect_oracles.c brings oracle/pt_oracle.c, the camera, query and AO restatements and both illumination restatements whole;
 * mis_oracle.c builds on their statics.
 */
#include "indirect_oracles.c"
#include "mis_oracle.c"
