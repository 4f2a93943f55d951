/*
 * indirect_oracles.c -- the one translation unit of tests/libtest_indirect_oracle.so (tests/indirect_oracle.py builds it).
 * TEST INFRASTRUCTURE.  direct_oracles.c brings oracle/pt_oracle.c, the camera, query and AO restatements and direct
 * illumination's whole; indirect_oracle.c builds on their statics.
 */
#include "direct_oracles.c"
#include "indirect_oracle.c"
