// custom_sphere.h — the device side of custom-geometry sphere BLASes (kernels_custom.hip, and the sphere step of kernels_tlas.hip's flat loop).
//
// A sphere BLAS is the reference's BVH over custom geometry (BVH::Build( customGetAABB, n ), tiny_bvh.h:2190-2219): 32-byte Wald nodes
// {aabbMin, leftFirst, aabbMax, triCount} (a leaf iff triCount > 0; children leftFirst, leftFirst + 1: one 64-byte read) and, gathered at
// upload in primIdx order, one 32-byte record per index entry: {x, y, z, r}, {prim, 0, 0, 0}.
//
// The primitive test restates the callback of the reference's anim demo (tiny_bvh_anim.cpp:38-60), the form that stays right when D is not of
// unit length (a scaled instance), with the products its x86 build (-O3 -mavx2 -mfma) fuses — read from the disassembly of the callback as
// tests/custom_ref_shim.cpp compiles it — written as explicit fmas; the library builds with -ffp-contract=off, so nothing else is fused:
//   mag = sqrt(fma(D.z, D.z, fma(D.x, D.x, D.y D.y))), reciMag = 1 / mag            (correctly rounded sqrt and division)
//   oc = O - pos;  b = fma(oc.z, D.z, fma(oc.x, D.x, oc.y D.y)) * reciMag
//   c = fma(-r, r, fma(oc.z, oc.z, fma(oc.x, oc.x, oc.y oc.y)));  d = fma(b, b, -c)
//   miss if d <= 0; t = -b - sqrt(d); a candidate iff t < tmax_in * mag && t > 0; it records hit.t = t * reciMag
// tests/oracle_custom.c restates the same operations; the device matches it byte for byte.
#pragma once
#include "device_common.h"

namespace tbvh {

constexpr int kLayoutBvh2Wald = 1;   // TBVH_LAYOUT_BVH2_WALD: a sphere BLAS

// the per-ray (per-instance under a TLAS) factors of the callback: the same bits the reference recomputes for every sphere
struct SphereRay {
    float reciMag;   // 1 / |D|
    float tmaxMag;   // tmax_in * |D|: a candidate lies below it
};
__device__ __forceinline__ SphereRay sphere_ray(float3 D, float tmaxIn) {
    const float mag = __builtin_sqrtf(__builtin_fmaf(D.z, D.z, __builtin_fmaf(D.x, D.x, D.y * D.y)));
    SphereRay r;
    r.reciMag = 1.0f / mag;
    r.tmaxMag = tmaxIn * mag;
    return r;
}

// true: sphere s = {x, y, z, r} is a candidate; *stored = the distance it records (a ray parameter, t * reciMag)
__device__ __forceinline__ bool sphere_test(float3 O, float3 D, float4 s, const SphereRay& sr, float& stored) {
    const float ocx = O.x - s.x, ocy = O.y - s.y, ocz = O.z - s.z;
    const float b = __builtin_fmaf(ocz, D.z, __builtin_fmaf(ocx, D.x, ocy * D.y)) * sr.reciMag;
    const float c = __builtin_fmaf(-s.w, s.w, __builtin_fmaf(ocz, ocz, __builtin_fmaf(ocx, ocx, ocy * ocy)));
    const float d = __builtin_fmaf(b, b, -c);
    if (d <= 0.f) return false;
    const float t = -b - __builtin_sqrtf(d);
    if (!(t < sr.tmaxMag && t > 0.f)) return false;
    stored = t * sr.reciMag;
    return true;
}

// The library's winner rule for a sphere candidate (DESIGN.md par. 12): the smallest recorded distance, then the smaller primitive, then the
// smaller instance — the order of hit_wins, but complete: a candidate's recorded distance can lie beyond the closest hit so far (it is checked
// against the ray's INCOMING tmax, scaled by |D|, so that the answer does not depend on the visit order).
__device__ __forceinline__ bool sphere_wins(float t, uint32_t prim, uint32_t inst, bool found, float4 best, uint32_t bestInst) {
    if (!found || t < best.x) return true;
    if (!(t == best.x)) return false;
    const uint32_t bp = as_u32(best.w);
    return prim < bp || (prim == bp && inst < bestInst);
}

// SLAB_TEST_TWO_NODES (tiny_bvh.h:3202-3220) for one child: near / far planes by the sign of D, t = plane * rD - O rD fused, tmin clamped
// to 0, tmax to the cull bound; kFar when missed.  tinybvh_min / _max as the reference writes them (a < b ? a : b).
__device__ __forceinline__ float wald_slab(float4 lo, float4 hi, float3 rD, float3 ro, bool px, bool py, bool pz, float bound) {
    const float tx1 = __builtin_fmaf(px ? lo.x : hi.x, rD.x, -ro.x), tx2 = __builtin_fmaf(px ? hi.x : lo.x, rD.x, -ro.x);
    const float ty1 = __builtin_fmaf(py ? lo.y : hi.y, rD.y, -ro.y), ty2 = __builtin_fmaf(py ? hi.y : lo.y, rD.y, -ro.y);
    const float tz1 = __builtin_fmaf(pz ? lo.z : hi.z, rD.z, -ro.z), tz2 = __builtin_fmaf(pz ? hi.z : lo.z, rD.z, -ro.z);
    const float a = tx1 > ty1 ? tx1 : ty1, b = tz1 > 0.f ? tz1 : 0.f;
    const float tmin = a > b ? a : b;
    const float c = tx2 < ty2 ? tx2 : ty2, d = tz2 < bound ? tz2 : bound;
    const float tmax = c < d ? c : d;
    return tmax >= tmin ? tmin : kFar;
}

}  // namespace tbvh
