/*
 * power_oracles.c -- the one translation unit of tests/libtest_power_oracle.so (tests/power_oracle.py builds it).  TEST INFRASTRUCTURE.
 * The restatements power_oracle.c builds on, in tests/oracles.c's order (camera_oracle.c includes oracle/pt_oracle.c whole), then
 * power_oracle.c itself.
 */
#include "camera_oracle.c"
#include "direct_oracle.c"
#include "indirect_oracle.c"
#include "mis_oracle.c"
#include "power_oracle.c"
