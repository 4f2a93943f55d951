/*
 * env_oracles.c -- the one translation unit of tests/libtest_env_oracle.so (tests/env_oracle.py builds it).  TEST INFRASTRUCTURE.
 * The restatements env_oracle.c builds on, in tests/roulette_oracles.c's order (camera_oracle.c includes oracle/pt_oracle.c whole),
 * then env_oracle.c itself.
 */
#include "camera_oracle.c"
#include "direct_oracle.c"
#include "indirect_oracle.c"
#include "mis_oracle.c"
#include "power_oracle.c"
#include "roulette_oracle.c"
#include "env_oracle.c"
