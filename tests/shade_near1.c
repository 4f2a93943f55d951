/* The near-1 form of 1 / sqrt(x) (csrc/pt_device_math.h, pt_rsqrt_near1) restated in C: compile with -ffp-contract=off.
 * TEST INFRASTRUCTURE (tests/test_shade_near1_cpu.py).  Prints "<floats> <mismatches> <first failing bits>" for every binary32
 * whose bits lie in [argv[1], argv[2]] (hexadecimal), against 1.0f / sqrtf(x); argv[3] = 1 takes 1/2, 1/2 and 1 for the constants. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static float rsqrt_near1(float x, int plain)
{
    const float gc = plain ? 0.5f : 0x1.000002p-1f, h = plain ? 0.5f : 0x1.000002p-1f, yk = plain ? 1.0f : 0x1.fffffep-1f;
    const float g = fmaf(x, 0.5f, gc);
    const float rr = fmaf(-g, g, x);
    const float s = fmaf(rr, h, g);
    const float y = fmaf(-s, yk, 2.0f);
    const float e = fmaf(-s, y, 1.0f);
    return fmaf(e, y, y);
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const uint32_t lo = (uint32_t)strtoul(argv[1], 0, 16), hi = (uint32_t)strtoul(argv[2], 0, 16);
    const int plain = argc > 3 && atoi(argv[3]);
    unsigned long n = 0, bad = 0;
    uint32_t first = 0;
    for (uint32_t u = lo;; ++u) {
        const float x = from_bits(u);
        ++n;
        if (bits(rsqrt_near1(x, plain)) != bits(1.0f / sqrtf(x))) {
            if (!bad) first = u;
            ++bad;
        }
        if (u == hi) break;
    }
    printf("%lu %lu %08x\n", n, bad, first);
    return 0;
}
