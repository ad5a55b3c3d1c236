/* oracle_omm.c — TEST INFRASTRUCTURE ONLY: CreateOpacityMicroMap of the reference's tiny_scene.h (1682-1723) restated in plain C, independent of
 * tinybvh_amd/csrc/omm.h: the reference's own loops (u is a running sum, a row ends at the first u + v >= 1), its index formula and its texel fetch, with
 * the multiply-adds its build (g++ -O3 -mavx2 -mfma) fuses written as fmaf and nothing else allowed to fuse (-ffp-contract=off; tests/omm_lib.py).
 * tests/test_omm_host.py holds it to the real reference bit for bit.  Finite UVs only: the int conversions are the reference's. */
#include <math.h>
#include <stdint.h>
#include <string.h>

/* uv: nTris x 6 floats (u0 v0 u1 v1 u2 v2), triTexture: nTris u32 (0xFFFFFFFF = none), texels[k]: widths[k] x heights[k] u32;
 * out: nTris x ((N * N + 31) / 32) u32 */
void oorc_bake(const float* uv, uint32_t nTris, const uint32_t* triTexture, const uint32_t* const* texels, const uint32_t* widths, const uint32_t* heights,
               uint32_t nTextures, int N, uint32_t* out) {
    const float fN = (float)N;
    const float rN = 1.0f / fN;
    const int dwordsPerTri = (N * N + 31) >> 5;
    (void)nTextures;
    for (uint32_t i = 0; i < nTris; i++) {
        uint32_t* map = out + (size_t)i * dwordsPerTri;
        if (triTexture[i] == 0xFFFFFFFFu) { memset(map, 255, dwordsPerTri * 4); continue; }
        memset(map, 0, dwordsPerTri * 4);
        const uint32_t* pixels = texels[triTexture[i]];
        const int iw = (int)widths[triTexture[i]], ih = (int)heights[triTexture[i]];
        const float w = (float)widths[triTexture[i]], h = (float)heights[triTexture[i]];
        const float u0 = uv[6 * i + 0], v0 = uv[6 * i + 1], u1 = uv[6 * i + 2], v1 = uv[6 * i + 3], u2 = uv[6 * i + 4], v2 = uv[6 * i + 5];
        for (int y = 0; y < N * 4; y++) {
            const float v = ((float)y + 0.5f) * 0.25f * rN;
            float u = 0.125f / fN;
            for (int x = 0; x < N * 4; x++, u += 0.25f / fN) {
                if (u + v >= 1) break;
                const int row = (int)((u + v) * fN), diag = (int)((1 - u) * fN);
                const int idx = (row * row) + (int)(v * fN) + (diag - (N - 1 - row));
                const float b = (1 - u) - v;
                const float tu = fmaf(b, u0, fmaf(u, u1, v * u2));
                const float tv = fmaf(b, v0, fmaf(u, v1, v * v2));
                int iu = (int)((tu - floorf(tu)) * w), iv = (int)((tv - floorf(tv)) * h);
                if (iu > iw - 1) iu = iw - 1;
                if (iv > ih - 1) iv = ih - 1;
                const uint32_t pixel = pixels[iu + iv * iw];
                if ((pixel >> 24) > 2) map[idx >> 5] |= 1u << (idx & 31);
            }
        }
    }
}

/* how many samples of the textured triangles take the clamp to the last texel column or row (the fraction rounded to 1) */
uint32_t oorc_clamped(const float* uv, uint32_t nTris, const uint32_t* triTexture, const uint32_t* widths, const uint32_t* heights, int N) {
    const float fN = (float)N;
    uint32_t n = 0;
    for (uint32_t i = 0; i < nTris; i++) {
        if (triTexture[i] == 0xFFFFFFFFu) continue;
        const float w = (float)widths[triTexture[i]], h = (float)heights[triTexture[i]];
        const float u0 = uv[6 * i + 0], v0 = uv[6 * i + 1], u1 = uv[6 * i + 2], v1 = uv[6 * i + 3], u2 = uv[6 * i + 4], v2 = uv[6 * i + 5];
        for (int y = 0; y < N * 4; y++)
            for (int x = 0; x + y + 1 < N * 4; x++) {
                const float v = ((float)y + 0.5f) * 0.25f / fN, u = ((float)x + 0.5f) * 0.25f / fN, b = (1 - u) - v;
                const float tu = fmaf(b, u0, fmaf(u, u1, v * u2)), tv = fmaf(b, v0, fmaf(u, v1, v * v2));
                if ((int)((tu - floorf(tu)) * w) > (int)widths[triTexture[i]] - 1 || (int)((tv - floorf(tv)) * h) > (int)heights[triTexture[i]] - 1) n++;
            }
    }
    return n;
}
