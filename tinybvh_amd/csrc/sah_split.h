// sah_split.h — everything that decides a tree of the reference's default builder, BVH::Build( nodeIdx, depth ) (tiny_bvh.h:2332-2461, with
// PrepareBuild, 2261-2329), written once for the device builder (kernels_sahbuild.hip) and its host twin (sahbuild_host.cpp).  DESIGN.md §18.
//
// The arithmetic contract: every operation as the reference writes it, each rounded once (csrc is compiled with -ffp-contract=off), EXCEPT the
// two places where the reference build (gcc -O3 -mavx2 -mfma, default contraction) fuses, read from its disassembly and written out here:
//   - the half area x y + y z + z x of tinybvh_half_area and BVHBase::SA is fmaf( z, x, fmaf( x, y, y * z ) );
//   - the final cost c_trav + c_int * rSAV * splitCost is fmaf( c_int * rSAV, splitCost, c_trav ), with c_trav = c_int = 1.
// Reductions over primitives (triangle boxes into the root box and into bins) are mins and maxes taken in the total order of sah::key, in which
// -0 < +0: the result does not depend on the order of the primitives, which is what lets a parallel builder reproduce a sequential one.  (The
// reference's a < b ? a : b keeps whichever of -0 / +0 came last; a box face that meets both may differ from the reference's in that sign bit.)
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SAH_HD __host__ __device__ __forceinline__
#else
#define SAH_HD inline
#endif

namespace tbvh {
namespace sah {

constexpr int kBins = 8;          // BVHBINS
constexpr float kFar = 1e30f;     // BVH_FAR
constexpr int kBinWords = 7;      // per (axis, bin): min x y z, max x y z, count
constexpr int kNodeBinWords = 3 * kBins * kBinWords;

SAH_HD uint32_t f2u(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u; memcpy(&u, &f, 4); return u;
#endif
}
SAH_HD float u2f(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f; memcpy(&f, &u, 4); return f;
#endif
}
SAH_HD float fma1(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);
#else
    return fmaf(a, b, c);
#endif
}

// order-preserving float -> uint (a total order: -0 < +0), and back
SAH_HD uint32_t key(float f) { const uint32_t b = f2u(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
SAH_HD float unkey(uint32_t e) { return u2f((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }
SAH_HD float min_ord(float a, float b) { return key(b) < key(a) ? b : a; }
SAH_HD float max_ord(float a, float b) { return key(b) > key(a) ? b : a; }
// tinybvh_min / tinybvh_max (tiny_bvh.h:445-446): where the order of the operands is fixed by the code
SAH_HD float min_ref(float a, float b) { return a < b ? a : b; }
SAH_HD float max_ref(float a, float b) { return a > b ? a : b; }

// a fragment's box: componentwise tinybvh_min( v0, tinybvh_min( v1, v2 ) ) (PrepareBuild, 2303-2304)
SAH_HD void fragment_box(const float v0[3], const float v1[3], const float v2[3], float mn[3], float mx[3]) {
    for (int k = 0; k < 3; k++) { mn[k] = min_ref(v0[k], min_ref(v1[k], v2[k])); mx[k] = max_ref(v0[k], max_ref(v1[k], v2[k])); }
}

// the demos' sphereAABB for a record {x, y, z, r}: pos - bvhvec3( r ), pos + bvhvec3( r ), one rounding each (r <= 0 gives an inverted or empty box)
SAH_HD void sphere_box(const float s[4], float mn[3], float mx[3]) {
    for (int k = 0; k < 3; k++) { mn[k] = s[k] - s[3]; mx[k] = s[k] + s[3]; }
}

SAH_HD float half_area(float x, float y, float z) { return x < -kFar ? 0.f : fma1(z, x, fma1(x, y, y * z)); }

// rpd3 = bvhvec3( BVHBINS ) / (node.aabbMax - node.aabbMin) (2362)
SAH_HD float bin_scale(float nmin, float nmax) { return 8.0f / (nmax - nmin); }

// (int)( ((bmin + bmax) * 0.5f - nmin) * rpd ) clamped to 0..7 (2366-2369, 2419-2420).  A NaN product (0 x inf on a zero-extent axis), an infinite
// one and one beyond the int range convert to INT_MIN on x86, which clamps to bin 0: written out, not left to the conversion instruction.
SAH_HD int bin_index(float bmin, float bmax, float nmin, float rpd) {
    const float v = ((bmin + bmax) * 0.5f - nmin) * rpd;
    if (!(v > -2147483648.f && v < 2147483648.f)) return 0;
    const int b = (int)v;
    return b > 0 ? (b < kBins - 1 ? b : kBins - 1) : 0;
}

struct Split {
    uint32_t axis, pos;            // primitives whose bin on `axis` is <= pos go left
    float lmin[3], lmax[3], rmin[3], rmax[3];
};

// The per-axis sweep and the termination test (2378-2412).  B: bins.mn( a, i, k ), bins.mx( a, i, k ), bins.count( a, i ) — empty bins hold
// +/- BVH_FAR and 0.  minDim = (rootMax - rootMin) * 1e-20f.  false: not splitting is better (splitCost >= noSplitCost); the caller still
// makes a leaf when one side would be empty (2425).  The strict C < splitCost lets the first axis, then the first bin, win ties.
// A sweep in which NO candidate beat BVH_FAR — every axis behind the minDim gate, or every cost infinite — can still pass the termination test when the
// node's area is so large that rSAV * BVH_FAR is small (extents beyond 1e14): the reference then splits at axis 0, bin 0 and gives the children
// bestLMin .. bestRMax as an EARLIER node's sweep left them (2350: they live outside the loop).  first = this is the first node the reference
// evaluates (the root): they still hold their initial zeros, which is what the children get here.  For any later node they depend on the order of the
// sequential walk and are not reproduced: the children get the boxes of bin 0 and of bins 1 .. 7 on axis 0.
template <class B>
SAH_HD bool find_split(const B& bins, const float nmin[3], const float nmax[3], const float minDim[3], uint32_t triCount, bool first, Split& s) {
    float splitCost = kFar;
    const float rSAV = 1.0f / half_area(nmax[0] - nmin[0], nmax[1] - nmin[1], nmax[2] - nmin[2]);   // (BVHBase::SA: no BVH_FAR test, and an extent is never below it)
    uint32_t bestAxis = 0, bestPos = 0;
    bool found = false;
    for (int a = 0; a < 3; a++) if ((nmax[a] - nmin[a]) > minDim[a]) {
        // right-to-left: ANR[i] = area x count of bins i + 1 .. 7
        float ANR[kBins - 1];
        {
            float r1[3] = {kFar, kFar, kFar}, r2[3] = {-kFar, -kFar, -kFar};
            uint32_t rN = 0;
            for (int i = 0; i < kBins - 1; i++) {
                const int b = kBins - 1 - i;
                for (int k = 0; k < 3; k++) { r1[k] = min_ref(r1[k], bins.mn(a, b, k)); r2[k] = max_ref(r2[k], bins.mx(a, b, k)); }
                rN += bins.count(a, b);
                ANR[kBins - 2 - i] = rN == 0 ? kFar : (half_area(r2[0] - r1[0], r2[1] - r1[1], r2[2] - r1[2]) * (float)rN);
            }
        }
        float l1[3] = {kFar, kFar, kFar}, l2[3] = {-kFar, -kFar, -kFar};
        uint32_t lN = 0;
        for (int i = 0; i < kBins - 1; i++) {
            for (int k = 0; k < 3; k++) { l1[k] = min_ref(l1[k], bins.mn(a, i, k)); l2[k] = max_ref(l2[k], bins.mx(a, i, k)); }
            lN += bins.count(a, i);
            const float ANL = lN == 0 ? kFar : (half_area(l2[0] - l1[0], l2[1] - l1[1], l2[2] - l1[2]) * (float)lN);
            const float C = ANL + ANR[i];
            if (C < splitCost) splitCost = C, bestAxis = (uint32_t)a, bestPos = (uint32_t)i, found = true;
        }
    }
    splitCost = fma1(1.0f * rSAV, splitCost, 1.0f);
    const float noSplitCost = (float)triCount * 1.0f;
    if (splitCost >= noSplitCost) return false;
    // the child boxes are the sweep's own prefix / suffix boxes at the winning position (2402), taken again in the same order
    s.axis = bestAxis; s.pos = bestPos;
    if (!found && first) {
        for (int k = 0; k < 3; k++) s.lmin[k] = s.lmax[k] = s.rmin[k] = s.rmax[k] = 0.f;
        return true;
    }
    for (int k = 0; k < 3; k++) { s.lmin[k] = kFar; s.lmax[k] = -kFar; s.rmin[k] = kFar; s.rmax[k] = -kFar; }
    for (int i = 0; i <= (int)bestPos; i++)
        for (int k = 0; k < 3; k++) { s.lmin[k] = min_ref(s.lmin[k], bins.mn(bestAxis, i, k)); s.lmax[k] = max_ref(s.lmax[k], bins.mx(bestAxis, i, k)); }
    for (int b = kBins - 1; b > (int)bestPos; b--)
        for (int k = 0; k < 3; k++) { s.rmin[k] = min_ref(s.rmin[k], bins.mn(bestAxis, b, k)); s.rmax[k] = max_ref(s.rmax[k], bins.mx(bestAxis, b, k)); }
    return true;
}

// primitives on the left of a split: the counts of bins 0 .. pos on its axis
template <class B>
SAH_HD uint32_t left_count(const B& bins, const Split& s) {
    uint32_t n = 0;
    for (uint32_t i = 0; i <= s.pos; i++) n += bins.count((int)s.axis, (int)i);
    return n;
}

// BVH::SplitLeafs( k ) (1988-2017) turns a leaf of c > k primitives into a chain of this many extra node pairs: k go left, the rest right, again
SAH_HD uint32_t split_leaf_pairs(uint32_t count, uint32_t k) { return (k == 0 || count <= k) ? 0u : (count + k - 1) / k - 1; }

}  // namespace sah
}  // namespace tbvh
