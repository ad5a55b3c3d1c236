// shade.h — the arithmetic of the reference's GetShadingData (tiny_bvh_foliage.cpp:80-125): hit record -> instance -> FatTri -> material -> texel,
// float operation for float operation as that file's build (g++ -O3 -mavx2 -mfma) performs it (DESIGN.md par. 16).  One copy for the kernel
// (kernels_shade.hip) and the library's host path (capi_shade.hip: tbvh_host_shade_hits).  Everything that includes this is built -ffp-contract=off:
// the fused multiply-adds below are the ones the reference's object code has, and the only ones.
//
//   w = (1 - u) - v
//   tu = fma( w, u0, fma( u, u1, v * u2 ) ), tv likewise; t -= floorf( t )
//   iu = (int)( (float)width * tu ), iv = (int)( (float)height * tv ); index = (uint32)( iu + iv * width ), HERE clamped to width * height - 1
//   albedo = (float)byte * (1 / 256); alpha = byte 3 > 2 ? 1 : 0; untextured: the material's colour, alpha 1
//   transform_vector: r = fma( m[4r+2], z, fma( m[4r], x, m[4r+1] * y ) )
//   normalize: l2 = fma( z, z, fma( x, x, y * y ) ), l = sqrtf( l2 ), a * ( l == 0 ? 0 : 1 / l )      (IEEE sqrt and division)
//   dot( a, b ) = fma( a.z, b.z, fma( a.x, b.x, a.y * b.y ) ); N flips when dot( N, D ) > 0, iN when dot( iN, N ) < 0 (a NaN flips neither)
//   iN.k = fma( w, vN0.k, fma( v, vN2.k, u * vN1.k ) )
//   normal map: mN = fma( (float)byte, 1 / 128, -1 ) (exact either way: a byte times a power of two), iN.k = fma( mN.z, iN.k, fma( mN.y, B.k, mN.x * T.k ) )
//
// The one deliberate difference is the clamp: tu - floorf( tu ) is exactly 1.0f for a tiny negative tu, the reference then reads texel iu == width
// (the next row's first texel) or row `height` (past the allocation).  The clamped index equals the reference's wherever the reference's read is inside
// its array.  Nothing outside the tables is read whatever the records hold: every index is compared with its table's size before it becomes an address.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TBVH_SHADE_HD __host__ __device__ __forceinline__

namespace tbvh {

struct ShadeTex { const uint32_t* texels; uint32_t width, height; };    // tbvh_alpha_texture (width * height in [1, 2^31))
struct ShadeMat { float color[3]; uint32_t colorTex, normalTex; };      // tbvh_material
struct ShadeSlot { const float4* tris; uint64_t nTris; };               // one BLAS slot's FatTri records (12 float4 each); tris == nullptr: none
struct ShadeTables {
    const ShadeSlot* slots; const ShadeMat* mats; const ShadeTex* tex;
    uint32_t nSlots, nMats, nTex;
};
constexpr uint32_t kShadeNoTexture = 0xFFFFFFFFu;
constexpr uint32_t kShadeLayoutSphere = 1u, kShadeLayoutVoxel = 12u;   // TBVH_LAYOUT_BVH2_WALD / _VOXELSET: a hit on such a BLAS has no surface record, and that is no error

// the FatTri fields read here, as float4 q[12] of the 192-byte record (static_asserts on the real offsets: capi_shade.hip)
//   q0 = u0 u1 u2 ltriIdx | q1 = v0 v1 v2 material | q2 = vN0 Nx | q3 = vN1 Ny | q4 = vN2 Nz | q5..q7 = vertex0..2 | q8 = T area | q9 = B invArea
constexpr uint32_t kFatTriQuads = 12;

// the same builtins on both sides: correctly rounded on the host and, for a HIP compile without fast-math options (this library's), on the device —
// unlike __fsqrt_rn, which the HIP headers map to the approximate native square root
TBVH_SHADE_HD float shade_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
TBVH_SHADE_HD float shade_sqrt(float x) { return __builtin_sqrtf(x); }
TBVH_SHADE_HD float shade_rcp(float x) { return 1.0f / x; }
TBVH_SHADE_HD float shade_floor(float x) { return __builtin_floorf(x); }
TBVH_SHADE_HD float shade_bits_to_float(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(b);
#else
    float f; __builtin_memcpy(&f, &b, 4); return f;
#endif
}

TBVH_SHADE_HD uint32_t shade_float_to_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t b; __builtin_memcpy(&b, &f, 4); return b;
#endif
}

struct ShadeV3 { float x, y, z; };

TBVH_SHADE_HD float shade_dot(const ShadeV3& a, const ShadeV3& b) { return shade_fma(a.z, b.z, shade_fma(a.x, b.x, a.y * b.y)); }
TBVH_SHADE_HD ShadeV3 shade_transform_vector(const ShadeV3& a, const float4& m0, const float4& m1, const float4& m2) {
    ShadeV3 r;
    r.x = shade_fma(m0.z, a.z, shade_fma(m0.x, a.x, m0.y * a.y));
    r.y = shade_fma(m1.z, a.z, shade_fma(m1.x, a.x, m1.y * a.y));
    r.z = shade_fma(m2.z, a.z, shade_fma(m2.x, a.x, m2.y * a.y));
    return r;
}
TBVH_SHADE_HD ShadeV3 shade_normalize(const ShadeV3& a) {
    const float l = shade_sqrt(shade_fma(a.z, a.z, shade_fma(a.x, a.x, a.y * a.y)));
    const float rl = l == 0 ? 0.f : shade_rcp(l);
    ShadeV3 r = {a.x * rl, a.y * rl, a.z * rl};
    return r;
}
TBVH_SHADE_HD ShadeV3 shade_neg(const ShadeV3& a) { ShadeV3 r = {-a.x, -a.y, -a.z}; return r; }

// the texel a (tu, tv) in [0, 1] reads: the reference's linear index, clamped into the texture.  (int)x of the reference is defined for the products a
// finite UV gives; anything else (a NaN, or beyond the int range) indexes texel 0's row / column here instead of being undefined
TBVH_SHADE_HD int shade_to_int(float x) { return x >= 0.f && x < 2147483648.f ? (int)x : 0; }
TBVH_SHADE_HD uint32_t shade_texel_index(float tu, float tv, uint32_t width, uint32_t height) {
    const uint32_t iv = (uint32_t)shade_to_int((float)height * tv);
    const uint32_t iu = (uint32_t)shade_to_int((float)width * tu);
    const uint32_t idx = iu + iv * width, last = width * height - 1u;
    return idx < last ? idx : last;
}

TBVH_SHADE_HD void shade_no_surface(float4 out[3]) {
    out[0] = make_float4(0.f, 0.f, 0.f, -1.f);
    out[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    out[2] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// One hit record -> its 48 bytes.  r1, r3: float4 1 and 3 of the ray record (D; t u v prim), inst: the dword at byte 44.  instances: the TLAS's
// 192-byte records as float4[12] (transform rows in 0..3, blasIdx the last dword of float4 8), or nullptr: a single BLAS, taken as instance 0 of slot 0
// with the identity matrix.  blasLayout: the TBVH_LAYOUT_* of BLAS i at dword i * blasStride (the TLAS's descriptors), or nullptr.  Returns false when an
// index was out of range (the record is then "no surface", or — a bad material or texture index — shaded as untextured with albedo 0).
TBVH_SHADE_HD bool shade_hit(const ShadeTables& tb, const float4* instances, uint64_t nInst, const uint32_t* blasLayout, uint32_t blasStride, uint32_t nBlas,
                             const float4& r1,
                             uint32_t inst, const float4& r3, float4 out[3]) {
    shade_no_surface(out);
    if (r3.x >= 1e30f) return true;   // a miss
    const float u = r3.y, v = r3.z;
    const uint32_t primIdx = shade_float_to_bits(r3.w);
    float4 m0 = make_float4(1.f, 0.f, 0.f, 0.f), m1 = make_float4(0.f, 1.f, 0.f, 0.f), m2 = make_float4(0.f, 0.f, 1.f, 0.f);
    uint32_t slot = 0;
    if (instances) {
        if (inst >= nInst) return false;
        const float4* I = instances + 12 * (uint64_t)inst;
        m0 = I[0]; m1 = I[1]; m2 = I[2];
        slot = ((const uint32_t*)I)[35];
    }
    if (blasLayout) {
        if (slot >= nBlas) return false;
        const uint32_t layout = blasLayout[(uint64_t)slot * blasStride];
        if (layout == kShadeLayoutSphere || layout == kShadeLayoutVoxel) return true;
    }
    if (slot >= tb.nSlots) return false;
    const ShadeSlot s = tb.slots[slot];
    if (!s.tris || primIdx >= s.nTris) return false;
    const float4* q = s.tris + kFatTriQuads * (uint64_t)primIdx;
    const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4];
    bool ok = true;
    const uint32_t matIdx = shade_float_to_bits(q1.w);
    ShadeMat mat = {{0.f, 0.f, 0.f}, kShadeNoTexture, kShadeNoTexture};
    if (matIdx < tb.nMats) mat = tb.mats[matIdx]; else ok = false;
    if (mat.colorTex != kShadeNoTexture && mat.colorTex >= tb.nTex) { mat = ShadeMat{{0.f, 0.f, 0.f}, kShadeNoTexture, kShadeNoTexture}; ok = false; }
    if (mat.normalTex != kShadeNoTexture && mat.normalTex >= tb.nTex) { mat.normalTex = kShadeNoTexture; ok = false; }

    const float w = (1.f - u) - v;
    float tu = shade_fma(w, q0.x, shade_fma(u, q0.y, v * q0.z));
    float tv = shade_fma(w, q1.x, shade_fma(u, q1.y, v * q1.z));
    tu = tu - shade_floor(tu); tv = tv - shade_floor(tv);
    float ax = mat.color[0], ay = mat.color[1], az = mat.color[2], alpha = 1.f;
    uint32_t texel = 0;
    if (mat.colorTex != kShadeNoTexture) {
        const ShadeTex t = tb.tex[mat.colorTex];
        texel = t.texels[shade_texel_index(tu, tv, t.width, t.height)];
        ax = (float)(texel & 255u) * (1.0f / 256.0f);
        ay = (float)((texel >> 8) & 255u) * (1.0f / 256.0f);
        az = (float)((texel >> 16) & 255u) * (1.0f / 256.0f);
        alpha = (texel >> 24) > 2u ? 1.f : 0.f;
    }
    // the geometric normal, to world space
    ShadeV3 N = {q2.w, q3.w, q4.w};
    N = shade_normalize(shade_transform_vector(N, m0, m1, m2));
    const ShadeV3 D = {r1.x, r1.y, r1.z};
    if (shade_dot(N, D) > 0.f) N = shade_neg(N);
    // the interpolated normal, bent by the normal map, to world space
    ShadeV3 iN;
    iN.x = shade_fma(w, q2.x, shade_fma(v, q4.x, u * q3.x));
    iN.y = shade_fma(w, q2.y, shade_fma(v, q4.y, u * q3.y));
    iN.z = shade_fma(w, q2.z, shade_fma(v, q4.z, u * q3.z));
    if (mat.normalTex != kShadeNoTexture) {
        const ShadeTex t = tb.tex[mat.normalTex];
        const uint32_t px = t.texels[shade_texel_index(tu, tv, t.width, t.height)];
        const float mx = shade_fma((float)(px & 255u), 1.0f / 128.0f, -1.0f);
        const float my = shade_fma((float)((px >> 8) & 255u), 1.0f / 128.0f, -1.0f);
        const float mz = shade_fma((float)((px >> 16) & 255u), 1.0f / 128.0f, -1.0f);
        const float4 T = q[8], B = q[9];
        iN.x = shade_fma(mz, iN.x, shade_fma(my, B.x, mx * T.x));
        iN.y = shade_fma(mz, iN.y, shade_fma(my, B.y, mx * T.y));
        iN.z = shade_fma(mz, iN.z, shade_fma(my, B.z, mx * T.z));
    }
    iN = shade_normalize(shade_transform_vector(iN, m0, m1, m2));
    if (shade_dot(iN, N) < 0.f) iN = shade_neg(iN);
    out[0] = make_float4(ax, ay, az, alpha);
    out[1] = make_float4(N.x, N.y, N.z, q1.w);
    out[2] = make_float4(iN.x, iN.y, iN.z, shade_bits_to_float(texel));
    return ok;
}

}  // namespace tbvh
