// omm.h — the arithmetic of the reference's CreateOpacityMicroMap (tiny_scene.h:1682-1723, the worker of Mesh::CreateOpacityMicroMaps): which bit of a
// triangle's opacity micromap a barycentric sample lands on and whether the texel under it is opaque, float operation for float operation as the
// reference's build performs them (DESIGN.md par. 15).  One copy for the kernel (kernels_omm.hip), the library's host path (omm_host.cpp) and, through
// that, the tests.  Everything that includes this is built -ffp-contract=off: the four fused multiply-adds below are the only ones.
//
//   grid    v = (y + 0.5) * 0.25 / N, u = (x + 0.5) * 0.25 / N for x, y in [0, 4N); a row ends at the first u + v >= 1, i.e. the samples are those
//           with x + y + 1 < 4N: (4N - 1) * 2N of them
//   bit     row = int( (u + v) * N ), diag = int( (1 - u) * N ), idx = row * row + int( v * N ) + (diag - (N - 1 - row))      (Gruen et al. 2020)
//   texel   w = (1 - u) - v;  tu = fma( w, u0, fma( u, u1, v * u2 ) ), tv = fma( w, v0, fma( u, v1, v * v2 ) )
//           iu = min( width - 1, int( (tu - floorf( tu )) * float( width ) ) ), iv likewise; opaque when texels[iu + iv * width] >> 24 > 2
//
// N is a power of two from 1 to 64 (omm_valid_n).  For these every product and sum of the grid and the bit index is exact in fp32 — u, v, 1 - u - v are
// multiples of 2^-9 below 1, the products with N are multiples of 1/8 —, so the closed form above equals the reference's running sum u += 0.25f / fN,
// and idx = row^2 + (a number in [0, 2 row]) < N^2: a sample never lands outside its triangle's words.  For other N the reference's own idx can reach
// N^2 by rounding, which is why they are refused.  The only rounding left is in tu / tv.
//
// Where the reference is undefined this header is not: a non-finite UV makes (tu - floorf( tu )) a NaN, whose int conversion the reference leaves to
// the machine (and then indexes the texture with); omm_texel maps it to texel 0, clamps on both sides, and never converts a float outside int's range.
#pragma once
#include <stdint.h>

#include "../../include/tinybvh_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TBVH_OMM_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define TBVH_OMM_HD inline
#endif

namespace tbvh {

constexpr uint32_t kOmmNoTexture = 0xFFFFFFFFu;   // TBVH_OMM_NO_TEXTURE
constexpr uint32_t kOmmMaxN = 64;

struct OmmTex { const uint32_t* texels; uint32_t width, height; };   // tbvh_alpha_texture (width, height in [1, 2^31))
struct OmmUV { float u0, v0, u1, v1, u2, v2; };                     // the triangle's three corners

TBVH_OMM_HD bool omm_valid_n(uint32_t N) { return N >= 1 && N <= kOmmMaxN && (N & (N - 1)) == 0; }
TBVH_OMM_HD uint32_t omm_words(uint32_t N) { return (N * N + 31u) >> 5; }
TBVH_OMM_HD uint32_t omm_samples(uint32_t N) { return (4 * N - 1) * 2 * N; }

TBVH_OMM_HD float omm_fma(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);
#else
    return __builtin_fmaf(a, b, c);
#endif
}

// The samples of one triangle as a rectangle, for code that strides over them: row y holds 4N - 1 - y samples, so rows y and 4N - 2 - y together hold 4N.
// Line r in [0, 2N) holds row r in its first 4N - 1 - r columns and row 4N - 2 - r behind it; the last line (r = 2N - 1) is its own partner, so its second
// half holds nothing: false.
TBVH_OMM_HD bool omm_sample_xy(uint32_t N, uint32_t r, uint32_t c, uint32_t& x, uint32_t& y) {
    const uint32_t len = 4 * N - 1 - r;
    if (c < len) { x = c; y = r; return true; }
    x = c - len; y = 4 * N - 2 - r;
    return r != 2 * N - 1;
}

// texel coordinate of an interpolated UV: the reference's min( iw - 1, (int)((t - floorf( t )) * w) ), total
TBVH_OMM_HD uint32_t omm_texel(float t, uint32_t width) {
    const float p = (t - __builtin_floorf(t)) * (float)width;
    if (!(p >= 0.f)) return 0;                      // NaN (a non-finite UV)
    if (!(p < 2147483648.f)) return width - 1;
    const uint32_t i = (uint32_t)(int)p;
    return i < width - 1 ? i : width - 1;
}

// one sample (x + y + 1 < 4N) of a textured triangle: the bit it belongs to (< N * N), and whether the texel under it is opaque
TBVH_OMM_HD bool omm_sample(uint32_t N, uint32_t x, uint32_t y, const OmmUV& t, const OmmTex& tex, uint32_t& idx) {
    const float fN = (float)N, rN = 1.0f / fN;   // (a power of two: the reciprocal and the products with it are exact)
    const float v = ((float)y + 0.5f) * 0.25f * rN, u = ((float)x + 0.5f) * 0.25f * rN;
    const int row = (int)((u + v) * fN), diag = (int)((1 - u) * fN);
    idx = (uint32_t)((row * row) + (int)(v * fN) + (diag - ((int)N - 1 - row)));
    const float w = (1 - u) - v;
    const float tu = omm_fma(w, t.u0, omm_fma(u, t.u1, v * t.u2));
    const float tv = omm_fma(w, t.v0, omm_fma(u, t.v1, v * t.v2));
    const uint32_t iu = omm_texel(tu, tex.width), iv = omm_texel(tv, tex.height);
    const uint32_t pixel = tex.texels[iu + (uint64_t)iv * tex.width];
    return (pixel >> 24) > 2;
}

// a source as both sides read it (tbvh_omm_source with every pointer in the reader's memory)
struct OmmSrc {
    const char* uv; uint32_t uvStride; uint32_t nUV;   // two floats at uv + i * uvStride
    const uint32_t* indices;                           // 3 per triangle, or null: corners 3i .. 3i + 2
    const uint32_t* triTexture;                        // one per triangle, or null: texture 0
    const OmmTex* textures; uint32_t nTextures;
    uint64_t nTris;
};

// Triangle i's corners and texture (null: opaque).  Nothing outside the arrays is read whatever they hold: a corner index >= nUV is clamped to the last
// vertex, a texture index >= nTextures that is not kOmmNoTexture means no texture; `bad` is set for either.
TBVH_OMM_HD const OmmTex* omm_triangle(const OmmSrc& s, uint64_t i, OmmUV& t, bool& bad) {
    uint32_t c[3];
    for (int k = 0; k < 3; k++) {
        const uint64_t j = s.indices ? s.indices[3 * i + k] : 3 * i + k;
        if (j >= s.nUV) bad = true;
        c[k] = (uint32_t)(j < s.nUV ? j : s.nUV - 1);
    }
    const float* a = (const float*)(s.uv + (uint64_t)c[0] * s.uvStride);
    const float* b = (const float*)(s.uv + (uint64_t)c[1] * s.uvStride);
    const float* d = (const float*)(s.uv + (uint64_t)c[2] * s.uvStride);
    t.u0 = a[0]; t.v0 = a[1]; t.u1 = b[0]; t.v1 = b[1]; t.u2 = d[0]; t.v2 = d[1];
    const uint32_t ti = s.triTexture ? s.triTexture[i] : 0u;
    if (ti == kOmmNoTexture) return nullptr;
    if (ti >= s.nTextures) { bad = true; return nullptr; }
    return s.textures + ti;
}

// (omm_host.cpp) whole meshes on the CPU, under tbvh_host_bake_opacity_micromaps, which is defined there as well
int omm_check_source(const tbvh_omm_source* src, uint32_t N, const char* who, bool hostArrays);   // the header's validation rules; host arrays are range-checked
void omm_bake_host(const OmmSrc& s, uint32_t N, uint64_t first, uint64_t last, uint32_t* maps);            // triangles [first, last), the reference's loop order

}  // namespace tbvh
