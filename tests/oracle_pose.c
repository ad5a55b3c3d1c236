/* oracle_pose.c — TEST INFRASTRUCTURE ONLY: the vertex part of the reference's Mesh::SetPose( skin ) and Mesh::SetPose( weights ) (tiny_scene.h)
 * restated in plain C, independent of tinybvh_amd/csrc/pose.h.  Built -ffp-contract=off: the fused multiply-adds the reference's build performs
 * (DESIGN.md par. 14) are the explicit fmaf calls below and nothing else fuses. */
#include <math.h>
#include <stdint.h>

/* rest16: n x 4 floats (w ignored), joints4: n x 4, weights16: n x 4, mats16: row-major 4 x 4 per joint; out16: n x 4 */
void porc_skin(const float* rest16, uint32_t n, const uint32_t* joints4, const float* weights16, const float* mats16, float* out16) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* j = joints4 + 4 * (uint64_t)i;
        const float* w = weights16 + 4 * (uint64_t)i;
        const float x = rest16[4 * (uint64_t)i], y = rest16[4 * (uint64_t)i + 1], z = rest16[4 * (uint64_t)i + 2];
        float S[16], row[4];
        for (int c = 0; c < 16; c++) {
            float s = w[0] * mats16[16 * (uint64_t)j[0] + c];
            float p = w[1] * mats16[16 * (uint64_t)j[1] + c];
            s = s + p;
            p = w[2] * mats16[16 * (uint64_t)j[2] + c];
            s = s + p;
            p = w[3] * mats16[16 * (uint64_t)j[3] + c];
            s = s + p;
            S[c] = s;
        }
        for (int r = 0; r < 4; r++) {
            const float t = S[4 * r + 1] * y;
            row[r] = fmaf(S[4 * r + 2], z, fmaf(S[4 * r], x, t)) + S[4 * r + 3];
        }
        float* o = out16 + 4 * (uint64_t)i;
        if (row[3] == 1) { o[0] = row[0]; o[1] = row[1]; o[2] = row[2]; }
        else {
            const float inv = 1.0f / row[3];
            o[0] = row[0] * inv; o[1] = row[1] * inv; o[2] = row[2] * inv;
        }
        o[3] = 0;
    }
}

/* positions12: (n_targets + 1) arrays of n x 3 floats, array 0 the base; out16: n x 4 */
void porc_morph(const float* positions12, uint32_t n, uint32_t n_targets, const float* weights, float* out16) {
    for (uint32_t i = 0; i < n; i++) {
        float v[3];
        for (int k = 0; k < 3; k++) v[k] = positions12[3 * (uint64_t)i + k];
        for (uint32_t t = 1; t <= n_targets; t++)
            for (int k = 0; k < 3; k++) v[k] = fmaf(weights[t - 1], positions12[((uint64_t)t * n + i) * 3 + k], v[k]);
        float* o = out16 + 4 * (uint64_t)i;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = 1;
    }
}

/* how many vertices of a skin take the divide branch (row_3 != 1): the tests assert that their fixtures hold both kinds */
uint32_t porc_skin_divides(const float* rest16, uint32_t n, const uint32_t* joints4, const float* weights16, const float* mats16) {
    uint32_t count = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* j = joints4 + 4 * (uint64_t)i;
        const float* w = weights16 + 4 * (uint64_t)i;
        const float x = rest16[4 * (uint64_t)i], y = rest16[4 * (uint64_t)i + 1], z = rest16[4 * (uint64_t)i + 2];
        float S[4];
        for (int c = 0; c < 4; c++) {
            float s = w[0] * mats16[16 * (uint64_t)j[0] + 12 + c];
            float p = w[1] * mats16[16 * (uint64_t)j[1] + 12 + c];
            s = s + p;
            p = w[2] * mats16[16 * (uint64_t)j[2] + 12 + c];
            s = s + p;
            p = w[3] * mats16[16 * (uint64_t)j[3] + 12 + c];
            s = s + p;
            S[c] = s;
        }
        const float t = S[1] * y;
        const float row3 = fmaf(S[2], z, fmaf(S[0], x, t)) + S[3];
        if (row3 != 1) count++;
    }
    return count;
}
