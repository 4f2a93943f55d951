/*
 * roulette_oracles.c -- the one translation unit of tests/libtest_roulette_oracle.so (tests/roulette_oracle.py builds it).  TEST
 * INFRASTRUCTURE.  The restatements roulette_oracle.c builds on, in tests/power_oracles.c's order (camera_oracle.c includes
 * oracle/pt_oracle.c whole), then roulette_oracle.c itself.
 */
#include "camera_oracle.c"
#include "direct_oracle.c"
#include "indirect_oracle.c"
#include "mis_oracle.c"
#include "power_oracle.c"
#include "roulette_oracle.c"
