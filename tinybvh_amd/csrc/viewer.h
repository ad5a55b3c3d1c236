// viewer.h — what the reference's two CPU viewers do around Intersect and GetShadingData (tiny_bvh_gltf.cpp:76-86, 137-175; tiny_bvh_foliage.cpp:67-77,
// 128-190, triangle branch): the row-major pinhole generator of WorkerThread, SampleSky, the alpha-continue step, the sun term with its shadow ray, and
// the clamp-and-pack to 0x00BBGGRR.  One copy for the kernels (kernels_viewer.hip) and the library's host twins (capi_viewer.hip: tbvh_host_viewer_* /
// tbvh_host_sky_*).  Everything that includes this is built -ffp-contract=off: the fused multiply-adds below are the ones the reference's build
// (g++ -O3 -mavx2 -mfma, which contracts a product into the sum that is its only use) performs, and the only ones (DESIGN.md par. 22).
//
//   generator   u = (float)px / W, v = (float)py / H                                         (ray i is pixel ( i % W, i / W ))
//               P.k = fma( v, p3.k - p1.k, fma( u, p2.k - p1.k, p1.k ) ) - eye.k;  D = normalize( normalize( P ) )   (WorkerThread, then Ray's constructor)
//               rD = safercp( D ), hit.t = 1e30, mask 0xFFFF
//   SampleSky   p = atan2( D.z, D.x );  uf = fma( (float)w * ( p + ( p < 0 ? 2 pi : 0 ) ), INV2PI, -0.5 );  vf = fma( (float)h * acos( D.y ), INVPI, -0.5 )
//               idx = min( (uint)uf + (uint)vf * w, w * h - 1 );  result = texel.zyx
//   continue    I.k = fma( D.k, t, O.k );  O.k = fma( D.k, 1e-4, I.k );  hit = ( 1e30, 0, 0, 0 )                    (tiny_bvh_gltf.cpp:144-149)
//   gltf light  t >= 10000: SampleSky( D ).  d = dot( iN, D ), R.k = fma( -( 2 d ), iN.k, D.k ) (not normalised),
//               c.k = albedo.k * fma( 0.5, SampleSky( R ).k, max( 0.2, dot( iN, L ) ) )
//   foliage     t >= 10000: SampleSky( D ).  A masked texel (alpha 0) has albedo ( 1, 0, 1 ).  c.k = ( albedo.k * ( shaded ? 0.3 : 1 ) ) * ( 0.25 + max( 0.2, dot( iN, L ) ) )
//               shadow ray: I.k = fma( D.k, t, O.k ), O' = fma( L.k, 0.001, I.k ), D' = normalize( L ), tmax 1000; a pixel without a hit below 10000 gets a
//               null ray (tmax 0)
//   pack        E.k = min( c.k, 1 ) * 255;  (int)E.x + ( (int)E.y << 8 ) + ( (int)E.z << 16 )
//
// atan2 and acos are NOT libm's: vw_atan2f / vw_acosf below are polynomials in explicit fmaf with one correctly rounded division resp. square root, so
// that the device and the host compute the same bits.  Their distance from float64 libm is measured by tools/viewer_math_error.c (profiles/viewer.txt)
// and bounds the texels where this sky and the reference's can differ (DESIGN.md par. 22: the SKY_EDGE margin).
//
// Deliberate differences from the reference, all in SampleSky:
//   - D.y is clamped to [-1, 1] before acos (the reference's acosf returns NaN there and converts it to an index: undefined).
//   - a negative or non-finite coordinate converts to 0, as shade_to_int does (a NaN direction samples texel 0's row and column).
//   - nothing outside the w * h texels is ever read.
// An infinite direction component gives an unspecified texel of the sky.
#pragma once
#include "shade.h"

namespace tbvh {

constexpr uint32_t kViewerGltf = 0u, kViewerFoliage = 1u;        // TBVH_VIEWER_GLTF / _FOLIAGE
constexpr uint32_t kViewerMaxRounds = 8u;

struct ViewerCam { float eye[3], p1[3], p2[3], p3[3]; uint32_t width, height; };
struct ViewerSky { const float* pixels; uint32_t width, height; };   // SkyDome::pixels (3 floats per texel); pixels == nullptr: no sky, every sample is 0

TBVH_SHADE_HD float vw_abs(float x) { return __builtin_fabsf(x); }
TBVH_SHADE_HD bool vw_signbit(float x) { return (shade_float_to_bits(x) >> 31) != 0u; }
TBVH_SHADE_HD float vw_safercp(float x) {   // tinybvh_safercp (tiny_bvh.h:442)
    if (x > 1e-12f || x < -1e-12f) return 1.0f / x;
    return x >= 0 ? 1e30f : -1e30f;
}

// pi, pi / 2, pi / 4 as a float and what it lacks
constexpr float kVwPiHi = 3.14159274f, kVwPiLo = -8.74227766e-8f;
constexpr float kVwPio2Hi = 1.57079637f, kVwPio2Lo = -4.37113883e-8f;
constexpr float kVwPio4Hi = 0.785398185f, kVwPio4Lo = -2.18556941e-8f;

// atan2f: q = min / max of the magnitudes, or ( min - max ) / ( min + max ) beyond tan( pi / 8 ) — one division either way, |q| <= tan( pi / 8 ) —, then
// atan( q ) = q + q z A( z ), z = q^2 (A: degree 4, fitted on [0, tan^2( pi / 8 )]), then the octant.  atan2( +-0, +0 ) = +-0, atan2( +-0, -0 ) = +-pi.
TBVH_SHADE_HD float vw_atan2f(float y, float x) {
    if (x != x || y != y) return x + y;
    const float ax = vw_abs(x), ay = vw_abs(y);
    const bool swap = ay > ax;
    const float a = swap ? ax : ay, b = swap ? ay : ax;
    const bool mid = a > 0.414213562f * b;
    float q = 0.f;
    if (b != 0.f) q = mid ? (a - b) / (a + b) : a / b;
    const float z = q * q;
    float p = shade_fma(z, -0.0643203035f, 0.107389368f);
    p = shade_fma(z, p, -0.14263688f);
    p = shade_fma(z, p, 0.199995428f);
    p = shade_fma(z, p, -0.333333313f);
    float r = shade_fma(q * z, p, q);
    if (mid) r = kVwPio4Hi + (r + kVwPio4Lo);
    if (swap) r = kVwPio2Hi - (r - kVwPio2Lo);
    if (vw_signbit(x)) r = kVwPiHi - (r - kVwPiLo);
    return vw_signbit(y) ? -r : r;
}

// acosf on [-1, 1]: asin( x ) = x + x z P( z ) with z = x^2 up to |x| = 0.5, beyond that z = ( 1 - |x| ) / 2 and acos( |x| ) = 2 asin( sqrt( z ) ) — one square
// root (P: degree 5, fitted on [0, 0.25]).  The caller clamps; a NaN comes back as a NaN.
TBVH_SHADE_HD float vw_asin_poly(float z) {
    float p = shade_fma(z, 0.0353269726f, 0.016190473f);
    p = shade_fma(z, p, 0.0312957317f);
    p = shade_fma(z, p, 0.0445833392f);
    p = shade_fma(z, p, 0.0750014037f);
    p = shade_fma(z, p, 0.166666657f);
    return z * p;
}
TBVH_SHADE_HD float vw_acosf(float x) {
    const float ax = vw_abs(x);
    if (!(ax > 0.5f)) {
        const float xr = x * vw_asin_poly(x * x);
        return kVwPio2Hi - (x - (kVwPio2Lo - xr));
    }
    const float z = (1.0f - ax) * 0.5f;
    const float s = shade_sqrt(z), r = vw_asin_poly(z);
    if (x < 0.f) {
        const float w = shade_fma(r, s, -kVwPio2Lo);
        return 2.0f * (kVwPio2Hi - (s + w));
    }
    return 2.0f * shade_fma(s, r, s);
}

// (uint32_t)x of the reference for the coordinates a finite direction gives (x > -1: truncation toward zero is defined); anything else converts to 0
TBVH_SHADE_HD uint32_t vw_to_uint(float x) { return x >= 0.f && x < 4294967296.f ? (uint32_t)x : 0u; }

constexpr float kVwInvPi = 0.31830988618379067153777f, kVwInv2Pi = 0.15915494309189533576888f, kVwTwoPi = 3.14159265358979323846264f * 2;

// the two texel coordinates before the conversion (the tests' restatement computes the same in float64 and marks the ones near an integer)
TBVH_SHADE_HD void vw_sky_coords(const ShadeV3& D, uint32_t w, uint32_t h, float* uf, float* vf) {
    const float p = vw_atan2f(D.z, D.x);
    const float y = D.y < -1.f ? -1.f : (D.y > 1.f ? 1.f : D.y);
    *uf = shade_fma((float)(int)w * (p + (p < 0.f ? kVwTwoPi : 0.f)), kVwInv2Pi, -0.5f);
    *vf = shade_fma((float)(int)h * vw_acosf(y), kVwInvPi, -0.5f);
}
TBVH_SHADE_HD uint32_t vw_sky_index(const ShadeV3& D, uint32_t w, uint32_t h) {
    float uf, vf;
    vw_sky_coords(D, w, h, &uf, &vf);
    const uint32_t idx = vw_to_uint(uf) + vw_to_uint(vf) * w, last = w * h - 1u;
    return idx < last ? idx : last;
}
// SampleSky: the texel as ( z, y, x ); *index (optional) = the texel read
TBVH_SHADE_HD ShadeV3 vw_sample_sky(const ViewerSky& sky, const ShadeV3& D, uint32_t* index = nullptr) {
    ShadeV3 r = {0.f, 0.f, 0.f};
    if (index) *index = 0u;
    if (!sky.pixels) return r;
    const uint32_t idx = vw_sky_index(D, sky.width, sky.height);
    const float* t = sky.pixels + 3 * (uint64_t)idx;
    r.x = t[2]; r.y = t[1]; r.z = t[0];
    if (index) *index = idx;
    return r;
}

// WorkerThread's ray for pixel i of a width x height image, as the four float4 of its record
TBVH_SHADE_HD void vw_generate(const ViewerCam& c, uint64_t i, float4 rec[4]) {
    const uint32_t px = (uint32_t)(i % c.width), py = (uint32_t)(i / c.width);
    const float u = (float)(int)px / (float)(int)c.width, v = (float)(int)py / (float)(int)c.height;
    ShadeV3 P;
    P.x = shade_fma(v, c.p3[0] - c.p1[0], shade_fma(u, c.p2[0] - c.p1[0], c.p1[0])) - c.eye[0];
    P.y = shade_fma(v, c.p3[1] - c.p1[1], shade_fma(u, c.p2[1] - c.p1[1], c.p1[1])) - c.eye[1];
    P.z = shade_fma(v, c.p3[2] - c.p1[2], shade_fma(u, c.p2[2] - c.p1[2], c.p1[2])) - c.eye[2];
    const ShadeV3 D = shade_normalize(shade_normalize(P));
    rec[0] = make_float4(c.eye[0], c.eye[1], c.eye[2], shade_bits_to_float(0xFFFFu));
    rec[1] = make_float4(D.x, D.y, D.z, 0.f);
    rec[2] = make_float4(vw_safercp(D.x), vw_safercp(D.y), vw_safercp(D.z), 0.f);
    rec[3] = make_float4(1e30f, 0.f, 0.f, 0.f);
}

// tiny_bvh_gltf.cpp's alpha rule on a 48-byte shading record: the hit is on a colour-textured material and its texel has x + y + z <= 5.  The material
// index is compared with the table's size before it is used; "no surface" (alpha -1) is never masked.
TBVH_SHADE_HD bool vw_gltf_masked(const ShadeMat* mats, uint32_t nMats, uint32_t nTex, const float4& o0, const float4& o1, const float4& o2) {
    if (o0.w < 0.f) return false;
    const uint32_t m = shade_float_to_bits(o1.w);
    if (m >= nMats) return false;
    const uint32_t ct = mats[m].colorTex;
    if (ct == kShadeNoTexture || ct >= nTex) return false;
    const uint32_t texel = shade_float_to_bits(o2.w);
    return (texel & 255u) + ((texel >> 8) & 255u) + ((texel >> 16) & 255u) <= 5u;
}
// does the record go on to another round (tiny_bvh_gltf.cpp:143-148)
TBVH_SHADE_HD bool vw_continues(const ShadeMat* mats, uint32_t nMats, uint32_t nTex, const float4& r3, const float4& o0, const float4& o1, const float4& o2) {
    return r3.x < 10000.f && vw_gltf_masked(mats, nMats, nTex, o0, o1, o2);
}
// the continue step on a record's O and hit quarters
TBVH_SHADE_HD float4 vw_stepped_origin(const float4& O, const float4& D, float t) {
    return make_float4(shade_fma(D.x, 0.0001f, shade_fma(D.x, t, O.x)), shade_fma(D.y, 0.0001f, shade_fma(D.y, t, O.y)), shade_fma(D.z, 0.0001f, shade_fma(D.z, t, O.z)), O.w);
}
TBVH_SHADE_HD void vw_step_on(float4& O, const float4& D, float4& hit) {
    O = vw_stepped_origin(O, D, hit.x);
    hit = make_float4(1e30f, 0.f, 0.f, 0.f);
}

TBVH_SHADE_HD float vw_max(float a, float b) { return a > b ? a : b; }   // tinybvh_max / _min: the second operand when a is a NaN
TBVH_SHADE_HD float vw_min(float a, float b) { return a < b ? a : b; }

// the shadow ray of tiny_bvh_foliage.cpp:166-167 for a record (r0, r1, r3 = O, D, hit), or the null ray
TBVH_SHADE_HD void vw_shadow_ray(const float4& r0, const float4& r1, const float4& r3, const ShadeV3& L, float4 rec[4]) {
    if (!(r3.x < 10000.f)) {
        rec[0] = make_float4(0.f, 0.f, 0.f, shade_bits_to_float(0xFFFFu));
        rec[1] = make_float4(0.f, 0.f, 1.f, 0.f);
        rec[2] = make_float4(1e30f, 1e30f, 1.f, 0.f);
        rec[3] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float t = r3.x;
    const ShadeV3 D = shade_normalize(L);
    rec[0] = make_float4(shade_fma(L.x, 0.001f, shade_fma(r1.x, t, r0.x)), shade_fma(L.y, 0.001f, shade_fma(r1.y, t, r0.y)),
                         shade_fma(L.z, 0.001f, shade_fma(r1.z, t, r0.z)), shade_bits_to_float(0xFFFFu));
    rec[1] = make_float4(D.x, D.y, D.z, 0.f);
    rec[2] = make_float4(vw_safercp(D.x), vw_safercp(D.y), vw_safercp(D.z), 0.f);
    rec[3] = make_float4(1000.f, 0.f, 0.f, 0.f);
}

// one pixel's colour from its final record (r1, r3 = D, hit), its shading record and, in the foliage mode, its shadow ray's flag
TBVH_SHADE_HD ShadeV3 vw_light(uint32_t mode, const ViewerSky& sky, const float4& r1, const float4& r3, const float4& o0, const float4& o2, bool shaded, const ShadeV3& L) {
    const ShadeV3 D = {r1.x, r1.y, r1.z};
    if (!(r3.x < 10000.f)) return vw_sample_sky(sky, D);
    const ShadeV3 iN = {o2.x, o2.y, o2.z};
    const float sun = vw_max(0.2f, shade_dot(iN, L));
    ShadeV3 c;
    if (mode == kViewerGltf) {
        const float d2 = 2.0f * shade_dot(iN, D);
        const ShadeV3 R = {shade_fma(-d2, iN.x, D.x), shade_fma(-d2, iN.y, D.y), shade_fma(-d2, iN.z, D.z)};
        const ShadeV3 ind = vw_sample_sky(sky, R);
        c.x = o0.x * shade_fma(0.5f, ind.x, sun);
        c.y = o0.y * shade_fma(0.5f, ind.y, sun);
        c.z = o0.z * shade_fma(0.5f, ind.z, sun);
    } else {
        const bool masked = o0.w == 0.f;
        const float ax = masked ? 1.f : o0.x, ay = masked ? 0.f : o0.y, az = masked ? 1.f : o0.z;
        const float s = shaded ? 0.3f : 1.0f, f = 0.25f + sun;
        c.x = (ax * s) * f; c.y = (ay * s) * f; c.z = (az * s) * f;
    }
    return c;
}

// (int)x for the values min( c, 1 ) * 255 can take; beyond the int range (only far below zero): 0
TBVH_SHADE_HD uint32_t vw_to_int(float x) { return x > -2147483648.f ? (uint32_t)(int)x : 0u; }
TBVH_SHADE_HD uint32_t vw_pack(float cx, float cy, float cz) {
    const float ex = vw_min(cx, 1.f) * 255.0f, ey = vw_min(cy, 1.f) * 255.0f, ez = vw_min(cz, 1.f) * 255.0f;
    return vw_to_int(ex) + (vw_to_int(ey) << 8) + (vw_to_int(ez) << 16);
}

}  // namespace tbvh
