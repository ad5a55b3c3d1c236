// lbvh.h — the one copy of the Morton-sort / Karras 2012 LBVH core that the three device builders share: triangles, spheres and PLOC's keys
// (kernels_build.hip), the fp32 TLAS (kernels_tlasbuild.hip) and the fp64 TLAS (kernels_double_anim.hip).  DESIGN.md §3.6.
//
// Upper part: plain functions without HIP runtime calls, so the host runs them too (tbvh_debug_lbvh_topology, tests/test_lbvh_host.py): the
// order-preserving float encoding, bit spreading, Morton keys, the prefix length with its tie rule and the Karras range search.  Lower part,
// device only: the per-wave reduction of centre bounds and the agent-scope box load.  What a builder does with a node (its stores, its
// numbering, its bottom-up pass) stays in the builder's file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LBVH_HD __host__ __device__ __forceinline__
#else
#define LBVH_HD inline
#endif

namespace tbvh {
namespace lbvh {

// ---- order-preserving float -> unsigned, and back: a < b as floats <=> encode(a) < encode(b) (-0 below +0) ---------------------------------
LBVH_HD uint32_t ordered_encode(float f) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
LBVH_HD float ordered_decode(uint32_t e) { return __builtin_bit_cast(float, (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }
LBVH_HD uint64_t ordered_encode(double d) {
    const uint64_t b = __builtin_bit_cast(uint64_t, d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
LBVH_HD double ordered_decode(uint64_t e) { return __builtin_bit_cast(double, (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e); }

// ---- bit spreading -----------------------------------------------------------------------------------------------------------------------
LBVH_HD uint32_t spread10(uint32_t v) {   // 10 bits -> every third bit of 30
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
LBVH_HD uint64_t spread21(uint64_t v) {   // 21 bits -> every third bit of 63
    v &= 0x1fffffull;
    v = (v | (v << 32)) & 0x001f00000000ffffull;
    v = (v | (v << 16)) & 0x001f0000ff0000ffull;
    v = (v | (v << 8)) & 0x100f00f00f00f00full;
    v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}

// ---- Morton keys -------------------------------------------------------------------------------------------------------------------------
// The two precisions clamp differently and keep doing so: the float form lets a NaN through (the conversion below then decides), the double
// form turns it into 0 (kernels_double_anim.hip leaves a non-finite centre out of the bounds and gives it key 0).
LBVH_HD float clamp01(float u) { return u < 0 ? 0.f : (u > 1 ? 1.f : u); }
LBVH_HD double clamp01(double u) { return u > 0 ? (u < 1 ? u : 1.) : 0.; }

// the cell 0 .. maxq of coordinate c within [lo, hi]: divide, clamp, scale, convert, min — each rounded once (-ffp-contract=off).  (The
// product is within [0, maxq] <= 2^21 - 1 or NaN, so the conversion to 32 bits gives what a conversion to 64 bits gives.)
template <class T>
LBVH_HD uint32_t morton_axis(T c, T lo, T hi, uint32_t maxq) {
    const T ext = hi - lo;
    const T u = clamp01(ext > 0 ? (c - lo) / ext : T(0));
    const uint32_t v = (uint32_t)(u * (T)maxq);
    return v > maxq ? maxq : v;
}
LBVH_HD uint32_t morton30(const uint32_t q[3]) { return (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]); }
LBVH_HD uint64_t morton63(const uint32_t q[3]) { return (spread21(q[0]) << 2) | (spread21(q[1]) << 1) | spread21(q[2]); }

// ---- prefix length -----------------------------------------------------------------------------------------------------------------------
LBVH_HD int clz32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz((int)x);
#else
    return x ? __builtin_clz(x) : 32;
#endif
}
LBVH_HD int clz64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return x ? __builtin_clzll(x) : 64;
#endif
}

// Karras 2012, "Maximizing parallelism in the construction of BVHs, octrees and k-d trees": the length of the common prefix of sorted keys i
// and j, -1 beyond the array.  The tie rule: equal keys are told apart by their position, as if each key were followed by its index.
template <class Key>
LBVH_HD int lbvh_delta(const Key* __restrict__ keys, int n, int i, int j) {
    constexpr int kKeyBits = 8 * (int)sizeof(Key);
    static_assert(kKeyBits == 32 || kKeyBits == 64, "32- or 64-bit keys");
    if (j < 0 || j >= n) return -1;
    const Key a = keys[i], b = keys[j];
    if (a == b) return kKeyBits + clz32((uint32_t)(i ^ j));
    return kKeyBits == 32 ? clz32((uint32_t)(a ^ b)) : clz64((uint64_t)(a ^ b));
}

// ---- topology ----------------------------------------------------------------------------------------------------------------------------
// Interior node i of the n - 1: its children in Karras ids (interior node g -> g, leaf g -> n - 1 + g) and its sorted range [lo, hi].
struct KarrasNode { uint32_t left, right, lo, hi; };

template <class Key>
LBVH_HD KarrasNode karras_node(const Key* __restrict__ keys, int n, int i) {
    const int d = lbvh_delta(keys, n, i, i + 1) - lbvh_delta(keys, n, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = lbvh_delta(keys, n, i, i - d);
    int lmax = 2;
    while (lbvh_delta(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (lbvh_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = lbvh_delta(keys, n, i, j);
    int s = 0;
    for (int t = (l + 1) >> 1;; t = (t + 1) >> 1) {
        if (lbvh_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    const int gamma = i + s * d + (d < 0 ? d : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    KarrasNode k;
    k.left = lo == gamma ? (uint32_t)(n - 1 + gamma) : (uint32_t)gamma;
    k.right = hi == gamma + 1 ? (uint32_t)(n - 1 + gamma + 1) : (uint32_t)(gamma + 1);
    k.lo = (uint32_t)lo; k.hi = (uint32_t)hi;
    return k;
}

#if defined(__HIPCC__)
// ==== device only =========================================================================================================================

// The centre bounds of the scene: every lane brings the bounds of the centres it has seen (lo > hi: none), the wave reduces them and lane 0
// issues ONE set of six atomics on the ordered encoding — the six words share a cache line, and same-line atomics are serialised memory-side
// (~12 ns each): one set per 64 triangles cost 3 ms for Bistro, one set per instance 70 of the 80 us of a 1000-instance TLAS rebuild.
// bounds: three minima, then three maxima (reset_centre_bounds, kernels.h).  Every lane of the wave must call.
// float: a wave without a centre is told by axis 0 alone (a lane has all three axes or none).
__device__ __forceinline__ void wave_centre_bounds(float lo[3], float hi[3], uint32_t* __restrict__ bounds) {
    for (int a = 0; a < 3; a++)
        for (int o = 32; o > 0; o >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], o)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o)); }
    if ((threadIdx.x & 63u) == 0 && lo[0] <= hi[0])
        for (int a = 0; a < 3; a++) { atomicMin(bounds + a, ordered_encode(lo[a])); atomicMax(bounds + 3 + a, ordered_encode(hi[a])); }
}
// double: told per axis, because the fp64 builder leaves a non-finite centre out per axis
__device__ __forceinline__ void wave_centre_bounds(double lo[3], double hi[3], uint64_t* __restrict__ bounds) {
    for (int a = 0; a < 3; a++)
        for (int o = 32; o > 0; o >>= 1) { lo[a] = fmin(lo[a], __shfl_xor(lo[a], o)); hi[a] = fmax(hi[a], __shfl_xor(hi[a], o)); }
    unsigned long long* b = (unsigned long long*)bounds;
    if ((threadIdx.x & 63u) == 0)
        for (int a = 0; a < 3; a++)
            if (lo[a] <= hi[a]) { atomicMin(b + a, (unsigned long long)ordered_encode(lo[a])); atomicMax(b + 3 + a, (unsigned long long)ordered_encode(hi[a])); }
}

// a box corner that a sibling on another CU wrote during this kernel: relaxed agent-scope loads bypass this CU's (non-coherent) L1
__device__ __forceinline__ float4 ld_agent(const float4* p) {
    const float* f = (const float*)p;
    return make_float4(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_load(f + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                       __hip_atomic_load(f + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0.f);
}
#endif

}  // namespace lbvh
}  // namespace tbvh
