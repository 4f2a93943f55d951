/* The guarded quotients of pt_shade's GGX branch (csrc/pt_device_math.h: pt_div, pt_div_pair) restated in C with the correctly
 * rounded reciprocal in pt_rcp_fast's place: compile with -ffp-contract=off.  TEST INFRASTRUCTURE (tests/test_shade_quotients_cpu.py).
 * What this can show without a GPU is that no exponent the guards admit breaks the three-instruction form -- q0, the residual and the
 * quotient stay normal over the whole window [2^-60, 2^60) of both operands -- and that the guards send everything else to "/".
 * That v_rcp_f32 plus one step IS the correctly rounded reciprocal over the window is the GPU tier's claim (mode 3).
 * Prints "<pairs> <inside the window> <mismatches>": binades 2^-61 .. 2^60 of both operands, argv[1] significand pairs each. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static int in_window(float x) { return bits(x) - 0x21800000u < 0x5d800000u - 0x21800000u; }
static float markstein(float a, float b)
{
    const float y = 1.0f / b;
    const float q0 = a * y;
    const float r = fmaf(-b, q0, a);
    return fmaf(r, y, q0);
}
static float div_guarded(float a, float b) { return in_window(a) && in_window(b) ? markstein(a, b) : a / b; }
static uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
static uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
static void div_pair(float a0, float b0, float a1, float b1, float* q0, float* q1)
{
    const uint32_t hi = umax(umax(bits(a1), bits(b0)), bits(b1)), lo = umin(umin(bits(a0), bits(b0)), bits(b1));
    if (hi < 0x5d800000u && lo >= 0x21800000u) { *q0 = markstein(a0, b0); *q1 = markstein(a1, b1); }
    else { *q0 = a0 / b0; *q1 = a1 / b1; }
}
static int differ(float got, float want) { return !((got != got && want != want) || bits(got) == bits(want)); }

int main(int argc, char** argv)
{
    const unsigned nsig = argc > 1 ? (unsigned)atoi(argv[1]) : 256u;
    unsigned long n = 0, inside = 0, bad = 0;
    uint32_t h = 20261018u;
    for (unsigned ea = 127 - 61; ea <= 127 + 60; ++ea)
        for (unsigned eb = 127 - 61; eb <= 127 + 60; ++eb)
            for (unsigned k = 0; k < nsig; ++k) {
                h = h * 1664525u + 1013904223u; const uint32_t ma = (h >> 9);
                h = h * 1664525u + 1013904223u; const uint32_t mb = (h >> 9);
                h = h * 1664525u + 1013904223u; const uint32_t mb2 = (h >> 9), eb2 = 127 - 61 + (h & 0xffu) % 122u;
                h = h * 1664525u + 1013904223u; const float c = (k & 7u) == 5u ? 1.0f : (k & 7u) == 6u ? 0.0f : (float)(h >> 8) * 0x1p-24f;
                float a = from_bits((ea << 23) | (k == 0 || k == 2 ? 0u : k == 1 || k == 3 ? 0x7fffffu : ma));
                const float b = from_bits((eb << 23) | (k == 0 || k == 3 ? 0u : k == 1 || k == 2 ? 0x7fffffu : mb));
                const float b2 = from_bits((eb2 << 23) | mb2);
                if (k == 4) a = 0.0f;
                ++n;
                inside += in_window(a) && in_window(b);
                bad += differ(div_guarded(a, b), a / b);
                float q0, q1;
                div_pair(a * c, b, a, b2, &q0, &q1);
                bad += differ(q0, a * c / b) + differ(q1, a / b2);
                if (k == 4) bad += differ(markstein(a, b), a / b);   /* a +0 numerator through the short form itself (pt_div_by) */
            }
    printf("%lu %lu %lu\n", n, inside, bad);
    return 0;
}
