/* oracle_viewer.c — TEST INFRASTRUCTURE ONLY: a plain-C restatement of what the reference's two CPU viewers do around Intersect and GetShadingData
 * (tiny_bvh_gltf.cpp:76-86, 137-175; tiny_bvh_foliage.cpp:67-77, 128-190, triangle branch), written from those files and independent of
 * tinybvh_amd/csrc/viewer.h: the row-major generator, SampleSky with libm's atan2f / acosf, the continue step, the two light rules, the shadow ray and
 * the pack.  Built -ffp-contract=off (tests/viewer_lib.py); the fused multiply-adds are the ones the reference's build (g++ -O3 -mavx2 -mfma) performs.
 *
 * SampleSky here also computes both texel coordinates in float64 and reports, per direction and axis, the nearest integer and whether the coordinate lies
 * within `margin` of it (SKY_EDGE_U / SKY_EDGE_V): there a sky that takes its atan2 / acos from somewhere else may read the texel across that boundary.
 * margin_ulps is given by the caller (DESIGN.md par. 22 derives it from tools/viewer_math_error.c's measurement); it is scaled by the coordinate. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define PI 3.14159265358979323846264f
#define INVPI 0.31830988618379067153777f
#define INV2PI 0.15915494309189533576888f

enum { SKY_EDGE_U = 1, SKY_EDGE_V = 2, SKY_CLAMPED_Y = 4, SKY_NAN = 8 };

typedef struct { float x, y, z; } v3;

static float dot3(v3 a, v3 b) { return fmaf(a.z, b.z, fmaf(a.x, b.x, a.y * b.y)); }
static v3 normalize3(v3 a) {
    const float l = sqrtf(dot3(a, a)), rl = l == 0 ? 0 : 1.0f / l;
    const v3 r = {a.x * rl, a.y * rl, a.z * rl};
    return r;
}
static float safercp(float x) { return (x > 1e-12f || x < -1e-12f) ? 1.0f / x : (x >= 0 ? 1e30f : -1e30f); }
static uint32_t to_uint(float x) { return x >= 0.f && x < 4294967296.f ? (uint32_t)x : 0u; }
static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

/* rays: 16 floats per record */
void ovw_generate(const float* eye, const float* p1, const float* p2, const float* p3, uint32_t W, uint32_t H, uint64_t first, uint64_t n, float* rays) {
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t i = first + k;
        const int px = (int)(i % W), py = (int)(i / W);
        const float u = (float)px / (float)(int)W, v = (float)py / (float)(int)H;
        float P[3];
        for (int c = 0; c < 3; c++) P[c] = fmaf(v, p3[c] - p1[c], fmaf(u, p2[c] - p1[c], p1[c])) - eye[c];
        v3 D = {P[0], P[1], P[2]};
        D = normalize3(normalize3(D));
        float* r = rays + 16 * k;
        r[0] = eye[0]; r[1] = eye[1]; r[2] = eye[2]; r[3] = from_bits(0xFFFFu);
        r[4] = D.x; r[5] = D.y; r[6] = D.z; r[7] = 0;
        r[8] = safercp(D.x); r[9] = safercp(D.y); r[10] = safercp(D.z); r[11] = 0;
        r[12] = 1e30f; r[13] = r[14] = r[15] = 0;
    }
}

/* one direction: the texel index the libm path reads; *flags, *ku, *kv as described above */
static uint32_t sky_index(v3 D, uint32_t w, uint32_t h, double margin_ulps, uint32_t* flags, int64_t* ku, int64_t* kv) {
    uint32_t f = 0;
    float y = D.y;
    if (y < -1.f) { y = -1.f; f |= SKY_CLAMPED_Y; }
    if (y > 1.f) { y = 1.f; f |= SKY_CLAMPED_Y; }
    const float p = atan2f(D.z, D.x);
    const float uf = fmaf((float)(int)w * (p + (p < 0 ? PI * 2 : 0)), INV2PI, -0.5f);
    const float vf = fmaf((float)(int)h * acosf(y), INVPI, -0.5f);
    if (uf != uf || vf != vf) f |= SKY_NAN;
    const double p64 = atan2((double)D.z, (double)D.x);
    const double u64 = (double)(int)w * (p64 + (p64 < 0 ? (double)(PI * 2) : 0.0)) * (double)INV2PI - 0.5;
    const double v64 = (double)(int)h * acos((double)y) * (double)INVPI - 0.5;
    const double scale = margin_ulps * 1.1920928955078125e-7;   /* 2^-23 */
    *ku = *kv = 0;
    if (u64 == u64) {
        const double k = floor(u64 + 0.5);
        *ku = (int64_t)k;
        if (k >= 1.0 && fabs(u64 - k) <= scale * (u64 + 0.5)) f |= SKY_EDGE_U;
    }
    if (v64 == v64) {
        const double k = floor(v64 + 0.5);
        *kv = (int64_t)k;
        if (k >= 1.0 && fabs(v64 - k) <= scale * (v64 + 0.5)) f |= SKY_EDGE_V;
    }
    *flags = f;
    const uint32_t idx = to_uint(uf) + to_uint(vf) * w, last = w * h - 1u;
    return idx < last ? idx : last;
}

static v3 sample_sky(const float* pixels, uint32_t w, uint32_t h, v3 D, double margin_ulps, uint32_t* flags) {
    v3 r = {0, 0, 0};
    *flags = 0;
    if (!pixels) return r;
    int64_t ku, kv;
    const uint32_t idx = sky_index(D, w, h, margin_ulps, flags, &ku, &kv);
    r.x = pixels[3 * (uint64_t)idx + 2]; r.y = pixels[3 * (uint64_t)idx + 1]; r.z = pixels[3 * (uint64_t)idx];
    return r;
}

/* dirs: 4 floats each; out: texel.zyx and the index bits; flags, ku, kv per direction */
void ovw_sky(const float* pixels, uint32_t w, uint32_t h, const float* dirs, uint64_t n, double margin_ulps, float* out, uint32_t* flags, int64_t* ku, int64_t* kv) {
    for (uint64_t i = 0; i < n; i++) {
        const v3 D = {dirs[4 * i], dirs[4 * i + 1], dirs[4 * i + 2]};
        const uint32_t idx = sky_index(D, w, h, margin_ulps, flags + i, ku + i, kv + i);
        out[4 * i] = pixels[3 * (uint64_t)idx + 2]; out[4 * i + 1] = pixels[3 * (uint64_t)idx + 1]; out[4 * i + 2] = pixels[3 * (uint64_t)idx];
        out[4 * i + 3] = from_bits(idx);
    }
}

/* the gltf alpha rule and continue step, in place; materials: 5 words each (colour, colour texture, normal texture); went: one byte per record */
void ovw_continue(const uint32_t* materials5, uint32_t nMats, uint32_t nTex, float* rays, uint32_t strideFloats, const float* out48, uint64_t n, uint8_t* went) {
    for (uint64_t i = 0; i < n; i++) {
        float* r = rays + (uint64_t)strideFloats * i;
        const float* o = out48 + 12 * i;
        went[i] = 0;
        if (!(r[12] < 10000.f) || o[3] < 0) continue;
        const uint32_t m = bits(o[7]);
        if (m >= nMats) continue;
        const uint32_t ct = materials5[5 * m + 3];
        if (ct == 0xFFFFFFFFu || ct >= nTex) continue;
        const uint32_t t = bits(o[11]);
        if ((t & 255u) + ((t >> 8) & 255u) + ((t >> 16) & 255u) > 5u) continue;
        for (int c = 0; c < 3; c++) r[c] = fmaf(r[4 + c], 0.0001f, fmaf(r[4 + c], r[12], r[c]));
        r[12] = 1e30f; r[13] = r[14] = r[15] = 0;
        went[i] = 1;
    }
}

void ovw_shadow_rays(const float* rays, uint32_t strideFloats, uint64_t n, const float* L, float* shadow) {
    const v3 l = {L[0], L[1], L[2]};
    const v3 D = normalize3(l);
    for (uint64_t i = 0; i < n; i++) {
        const float* r = rays + (uint64_t)strideFloats * i;
        float* s = shadow + 16 * i;
        memset(s, 0, 64);
        s[3] = from_bits(0xFFFFu);
        if (!(r[12] < 10000.f)) { s[6] = 1.f; s[8] = s[9] = 1e30f; s[10] = 1.f; continue; }
        for (int c = 0; c < 3; c++) s[c] = fmaf(L[c], 0.001f, fmaf(r[4 + c], r[12], r[c]));
        s[4] = D.x; s[5] = D.y; s[6] = D.z;
        s[8] = safercp(D.x); s[9] = safercp(D.y); s[10] = safercp(D.z);
        s[12] = 1000.f;
    }
}

/* mode 0 gltf, 1 foliage; rgb: 4 floats per record; edge[i] = the SKY_* flags of every sky sample the pixel took, or-ed */
void ovw_light(uint32_t mode, const float* pixels, uint32_t w, uint32_t h, const float* rays, uint32_t strideFloats, const float* out48, const uint8_t* occ, uint64_t n,
               const float* L, double margin_ulps, float* rgb, uint32_t* edge) {
    const v3 l = {L[0], L[1], L[2]};
    for (uint64_t i = 0; i < n; i++) {
        const float* r = rays + (uint64_t)strideFloats * i;
        const float* o = out48 + 12 * i;
        const v3 D = {r[4], r[5], r[6]};
        uint32_t f = 0, f2 = 0;
        v3 c;
        if (!(r[12] < 10000.f)) c = sample_sky(pixels, w, h, D, margin_ulps, &f);
        else {
            const v3 iN = {o[8], o[9], o[10]};
            const float d = dot3(iN, l), sun = 0.2f > d ? 0.2f : d;
            if (mode == 0) {
                const float d2 = 2 * dot3(iN, D);
                const v3 R = {fmaf(-d2, iN.x, D.x), fmaf(-d2, iN.y, D.y), fmaf(-d2, iN.z, D.z)};
                const v3 ind = sample_sky(pixels, w, h, R, margin_ulps, &f2);
                c.x = o[0] * fmaf(0.5f, ind.x, sun); c.y = o[1] * fmaf(0.5f, ind.y, sun); c.z = o[2] * fmaf(0.5f, ind.z, sun);
            } else {
                const int masked = o[3] == 0.f;
                const float ax = masked ? 1.f : o[0], ay = masked ? 0.f : o[1], az = masked ? 1.f : o[2];
                const float s = (occ && occ[i]) ? 0.3f : 1.0f, k = 0.25f + sun;
                c.x = (ax * s) * k; c.y = (ay * s) * k; c.z = (az * s) * k;
            }
        }
        rgb[4 * i] = c.x; rgb[4 * i + 1] = c.y; rgb[4 * i + 2] = c.z; rgb[4 * i + 3] = 0;
        edge[i] = f | f2;
    }
}

static uint32_t to_int(float x) { return x > -2147483648.f ? (uint32_t)(int)x : 0u; }
void ovw_pack(const float* rgb, uint64_t n, uint32_t* pixels) {
    for (uint64_t i = 0; i < n; i++) {
        float e[3];
        for (int c = 0; c < 3; c++) e[c] = (rgb[4 * i + c] < 1.f ? rgb[4 * i + c] : 1.f) * 255.0f;
        pixels[i] = to_int(e[0]) + (to_int(e[1]) << 8) + (to_int(e[2]) << 16);
    }
}
