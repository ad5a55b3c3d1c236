/* viewer_math_error.c — how far viewer.h's vw_atan2f / vw_acosf (through tbvh_debug_viewer_math) are from float64 libm, in ulps of the float result:
 *   acos   every float in [-1, 1]
 *   atan2  10^8 seeded pairs (half of them uniform in a square, half with exponents spread over 2^-40 .. 2^40) plus the axis and sign cases
 * Appends both maxima to the file named on the command line (profiles/viewer.txt); DESIGN.md par. 22 derives the SKY_EDGE margin of the tests from them.
 *   cc -O2 -Iinclude tools/viewer_math_error.c -Ltinybvh_amd -ltinybvh_amd -Wl,-rpath,$PWD/tinybvh_amd -lm -o viewer_math_error && ./viewer_math_error profiles/viewer.txt */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tinybvh_amd_debug.h"

#define CHUNK (1u << 20)
static float A[CHUNK], B[CHUNK], R[CHUNK];

static double ulp_of(double exact) {   /* the spacing of floats at |exact| */
    int e;
    const double m = fabs(exact);
    if (m < 1.17549435e-38) return 1.4012984643e-45;
    frexp(m, &e);
    return ldexp(1.0, e - 24);
}
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni(void) { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }

int main(int argc, char** argv) {
    double worstAcos = 0, worstAtan = 0;
    float atAcos = 0, atY = 0, atX = 0;
    /* acos: every float from -1 to 1 by its bit pattern */
    uint64_t count = 0;
    for (int sign = 0; sign < 2; sign++) {
        uint32_t b = 0;
        const uint32_t last = 0x3F800000u;   /* 1.0f */
        while (b <= last) {
            uint32_t n = 0;
            for (; n < CHUNK && b <= last; n++, b++) { const uint32_t w = b | ((uint32_t)sign << 31); memcpy(&A[n], &w, 4); }
            if (tbvh_debug_viewer_math(1, A, NULL, n, R)) return 1;
            for (uint32_t i = 0; i < n; i++) {
                const double ex = acos((double)A[i]), err = fabs((double)R[i] - ex) / ulp_of(ex);
                if (err > worstAcos) { worstAcos = err; atAcos = A[i]; }
            }
            count += n;
        }
    }
    /* atan2 */
    const uint64_t pairs = 100000000ull;
    uint64_t done = 0;
    const float special[] = {0.f, -0.f, 1.f, -1.f, 1e-30f, -1e-30f, 1e30f, -1e30f, 0.41421357f, 0.41421354f, 2.4142135f, 1.17549435e-38f, -1.17549435e-38f};
    const uint32_t ns = sizeof special / sizeof special[0];
    while (done < pairs + ns * ns) {
        uint32_t n = 0;
        for (; n < CHUNK && done < pairs + ns * ns; n++, done++) {
            if (done < ns * ns) { A[n] = special[done / ns]; B[n] = special[done % ns]; }
            else if (done & 1) { A[n] = (float)(2 * uni() - 1); B[n] = (float)(2 * uni() - 1); }
            else {
                A[n] = (float)ldexp(2 * uni() - 1, (int)(rng() % 81) - 40);
                B[n] = (float)ldexp(2 * uni() - 1, (int)(rng() % 81) - 40);
            }
        }
        if (tbvh_debug_viewer_math(0, A, B, n, R)) return 1;
        for (uint32_t i = 0; i < n; i++) {
            const double ex = atan2((double)A[i], (double)B[i]);
            const double err = ex == 0 ? ((double)R[i] == 0 ? 0 : 1e9) : fabs((double)R[i] - ex) / ulp_of(ex);
            if (err > worstAtan) { worstAtan = err; atY = A[i]; atX = B[i]; }
        }
    }
    FILE* f = argc > 1 ? fopen(argv[1], "a") : stdout;
    if (!f) return 2;
    fprintf(f, "viewer_math_error: vw_acosf   max %.3f ulp over %llu floats in [-1, 1] (at x = %.9g)\n", worstAcos, (unsigned long long)count, atAcos);
    fprintf(f, "viewer_math_error: vw_atan2f  max %.3f ulp over %llu pairs (at y = %.9g, x = %.9g)\n", worstAtan, (unsigned long long)done, atY, atX);
    if (f != stdout) fclose(f);
    return 0;
}
