// device_common.h — shared device-side definitions for the gfx950 traversal kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tbvh {

constexpr float kFar = 1e30f;  // BVH_FAR, tiny_bvh.h:144

// 64-byte ray record == first 64 bytes of tinybvh::Ray (tiny_bvh.h:689-709) == device
// struct Ray (traverse.cl:11-17).  Read as four 16-byte loads per lane.
struct __attribute__((aligned(16))) RayRec {
    float4 O;   // xyz, w = mask (u32)
    float4 D;   // xyz, w = instIdx (u32)
    float4 rD;  // xyz, w = hit.inst (u32) / pad
    float4 hit; // t, u, v, prim (u32)
};
static_assert(sizeof(RayRec) == 64, "ray record is 64 bytes");

__device__ __forceinline__ uint32_t as_u32(float f) { return __float_as_uint(f); }
__device__ __forceinline__ float as_f32(uint32_t u) { return __uint_as_float(u); }

// Ray/triangle test with the arithmetic of MOLLER_TRUMBORE_TEST (tiny_bvh.h:1644-1656) and
// the explicit FMA contraction pattern shared with oracle/tbvh_oracle.c (orc_tri), which is
// the pattern g++ 11.4 -O3 -mfma picks for the reference build:
//   h = crossA(D,e2); a = dot_zxy(e1,h); u = f*dot_zxy(s,h); q = crossB(s,e1);
//   v = f*dot_zyx(D,q); t = f*dot_zxy(e2,q)
// The kernels are compiled with -ffp-contract=off so nothing else in here is fused, and
// 1/a is the correctly rounded IEEE division (hipcc default).  t,u,v are therefore
// bit-identical to the oracle, and to BVH::Intersect as built by oracle/Makefile.
struct TriHit { float t, u, v; };

__host__ __device__ __forceinline__ float3 crossA(float3 a, float3 b) {  // first product fused
    float3 r;
    r.x = __builtin_fmaf(a.y, b.z, -(a.z * b.y));
    r.y = __builtin_fmaf(a.z, b.x, -(a.x * b.z));
    r.z = __builtin_fmaf(a.x, b.y, -(a.y * b.x));
    return r;
}
__host__ __device__ __forceinline__ float3 crossB(float3 a, float3 b) {  // second product fused
    float3 r;
    r.x = __builtin_fmaf(-a.z, b.y, a.y * b.z);
    r.y = __builtin_fmaf(-a.x, b.z, a.z * b.x);
    r.z = __builtin_fmaf(-a.y, b.x, a.x * b.y);
    return r;
}
__host__ __device__ __forceinline__ float dot_zxy(float3 a, float3 b) {
    return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.x, b.x, a.y * b.y));
}
__host__ __device__ __forceinline__ float dot_zyx(float3 a, float3 b) {
    return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x));
}

// Opacity micromaps (BVHBase::SetOpacityMicroMaps, tiny_bvh.h:823-826): n x n bits per triangle; a hit whose
// barycentrics fall on a clear bit is no hit (IntersectTri / TriOccludes, tiny_bvh.h:8514-8522, 8562-8570).
struct Omm { const uint32_t* map; uint32_t n; };   // map == nullptr: none
__host__ __device__ __forceinline__ bool omm_opaque(Omm om, uint32_t prim, float u, float v) {
    const float fN = (float)om.n;
    const int row = (int)((u + v) * fN), diag = (int)((1 - u) * fN);
    const int idx = (row * row) + (int)(v * fN) + (diag - ((int)om.n - 1 - row));
    const uint32_t* m = om.map + (size_t)prim * ((om.n * om.n + 31u) >> 5);
    return (m[idx >> 5] >> (idx & 31)) & 1u;
}

// Returns true when the triangle {v0, e1, e2} is hit within [0, tmax] (both ends
// inclusive, like the reference: rejects only t < 0 || t > tmax) and, with opacity
// micromaps set, the hit point is opaque.
__host__ __device__ __forceinline__ bool tri_test(float3 O, float3 D, float3 v0, float3 e1, float3 e2,
                                         float tmax, TriHit& h, Omm om = Omm{nullptr, 0u}, uint32_t prim = 0u) {
    const float3 hh = crossA(D, e2);
    const float a = dot_zxy(e1, hh);
    if (__builtin_fabsf(a) < 0.000001f) return false;
    const float f = 1.0f / a;
    const float3 s = make_float3(O.x - v0.x, O.y - v0.y, O.z - v0.z);
    const float u = f * dot_zxy(s, hh);
    const float3 q = crossB(s, e1);
    const float v = f * dot_zyx(D, q);
    if (u < 0 || v < 0 || u + v > 1) return false;
    const float t = f * dot_zxy(e2, q);
    if (t < 0 || t > tmax) return false;
    if (om.map && !omm_opaque(om, prim, u, v)) return false;
    h.t = t; h.u = u; h.v = v;
    return true;
}

// The same test without a branch, for the wave-packet kernel (kernels_cwbvh_packet.hip): there all 64 lanes hold a ray and every triangle is tested by all of
// them, so the early-outs above skip no vector instruction once a single lane passes, and each costs the wave an exec save / restore and a branch on the
// scalar unit (53 scalar instructions and 6 branches per triangle with them: profiles/packet_scalar.txt).  a, f, u, v, t are computed unconditionally with
// the helpers and in the order of tri_test; the predicate is made of the same comparisons with the same negations, so a NaN or an infinity in a lane (f = inf
// behind an edge-on triangle, a NaN vertex) is rejected or accepted exactly as above, and t, u, v of an accepted hit are the same bits
// (tests/test_tri_flat_host.py runs both forms on the host).  h is written whether or not the test passes.
__host__ __device__ __forceinline__ bool tri_test_flat(float3 O, float3 D, float3 v0, float3 e1, float3 e2,
                                                       float tmax, TriHit& h, Omm om = Omm{nullptr, 0u}, uint32_t prim = 0u) {
    const float3 hh = crossA(D, e2);
    const float a = dot_zxy(e1, hh);
    const float f = 1.0f / a;
    const float3 s = make_float3(O.x - v0.x, O.y - v0.y, O.z - v0.z);
    const float u = f * dot_zxy(s, hh);
    const float3 q = crossB(s, e1);
    const float v = f * dot_zyx(D, q);
    const float t = f * dot_zxy(e2, q);
    const bool edgeOn = __builtin_fabsf(a) < 0.000001f;
    const bool outside = (u < 0) | (v < 0) | (u + v > 1);
    const bool beyond = (t < 0) | (t > tmax);
    bool ok = !edgeOn & !outside & !beyond;
    if (om.map) ok = ok && omm_opaque(om, prim, u, v);
    h.t = t; h.u = u; h.v = v;
    return ok;
}

// ---- the watertight test (WATERTIGHT_TRITEST, tiny_bvh.h:8486-8507; Woop, Benthin, Wald 2013), a scene's choice (tbvh_set_triangle_test) ----------
// The ray's part, tiny_bvh.h:8489-8491: kz = the largest |D| component (tinybvh_maxdim), kx, ky the next two in cyclic order, swapped for D[kz] < 0;
// Sz = rD[kz] AS THE RAY RECORD HOLDS IT, Sx = D[kx] * Sz, Sy = D[ky] * Sz.
struct WtPre { uint32_t kx, ky, kz; float Sx, Sy, Sz; };
__host__ __device__ __forceinline__ float wt_axis(float3 v, uint32_t k) { return k == 0u ? v.x : (k == 1u ? v.y : v.z); }
__host__ __device__ __forceinline__ WtPre wt_precalc(float3 D, float3 rD) {
#pragma clang fp contract(off)
    WtPre p;
    const uint32_t r = __builtin_fabsf(D.x) > __builtin_fabsf(D.y) ? 0u : 1u;
    p.kz = __builtin_fabsf(D.z) > __builtin_fabsf(wt_axis(D, r)) ? 2u : r;
    p.kx = (1u << p.kz) & 3u; p.ky = (1u << p.kx) & 3u;
    if (wt_axis(D, p.kz) < 0) { const uint32_t s = p.kx; p.kx = p.ky; p.ky = s; }
    p.Sz = wt_axis(rD, p.kz); p.Sx = wt_axis(D, p.kx) * p.Sz; p.Sy = wt_axis(D, p.ky) * p.Sz;
    return p;
}
// The triangle's part, tiny_bvh.h:8493-8507, with EVERY product and sum rounded on its own (the region below says so whatever the file is compiled with): the
// edge function of an edge is then the exact negative of the same edge's function in the neighbouring triangle — the same two products, subtracted the other
// way round — so a ray cannot fall between the two.  Built with contraction (g++ -mfma fuses Cx * By - Cy * Bx) the reference's own test loses that and leaks
// (DESIGN.md par. 4.6).  Roles as IntersectTri has them: C = vC - O, A = vA - O, B = vB - O with (vC, vA, vB) = (v0, v1, v2), so u, v are the barycentrics of
// v1, v2 as in tri_test.  occRoles: TriOccludes' roles (tiny_bvh.h:8542-8544: A, B, C = v0, v1, v2), i.e. the caller passes (v2, v0, v1): the same three edge
// functions, summed in another order (det and T may round differently), and u, v are then taken from V, W, which are IntersectTri's U, V.
// Range of t: the library's, 0 <= t <= tmax (hit_wins decides among equal t), where tiny_bvh.h:8506 has t < tmax.  uvw: the three edge functions, for tests.
__host__ __device__ __forceinline__ bool tri_test_wt(float3 O, const WtPre& p, float3 vC, float3 vA, float3 vB, float tmax, TriHit& h, Omm om = Omm{nullptr, 0u},
                                                     uint32_t prim = 0u, bool occRoles = false, float* uvw = nullptr) {
#pragma clang fp contract(off)
    const float3 C = make_float3(vC.x - O.x, vC.y - O.y, vC.z - O.z);
    const float3 A = make_float3(vA.x - O.x, vA.y - O.y, vA.z - O.z);
    const float3 B = make_float3(vB.x - O.x, vB.y - O.y, vB.z - O.z);
    const float Akz = wt_axis(A, p.kz), Bkz = wt_axis(B, p.kz), Ckz = wt_axis(C, p.kz);
    const float Ax = wt_axis(A, p.kx) - p.Sx * Akz, Ay = wt_axis(A, p.ky) - p.Sy * Akz;
    const float Bx = wt_axis(B, p.kx) - p.Sx * Bkz, By = wt_axis(B, p.ky) - p.Sy * Bkz;
    const float Cx = wt_axis(C, p.kx) - p.Sx * Ckz, Cy = wt_axis(C, p.ky) - p.Sy * Ckz;
    const float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if (uvw) { uvw[0] = U; uvw[1] = V; uvw[2] = W; }
    if ((U < 0 || V < 0 || W < 0) && (U > 0 || V > 0 || W > 0)) return false;
    const float det = U + V + W;
    if (det == 0) return false;
    const float Az = p.Sz * Akz, Bz = p.Sz * Bkz, Cz = p.Sz * Ckz;
    const float T = U * Az + V * Bz + W * Cz;
    const float invDet = 1.0f / det, t = T * invDet;
    if (t < 0 || t > tmax) return false;
    const float u = (occRoles ? V : U) * invDet, v = (occRoles ? W : V) * invDet;
    // (a NaN vertex passes every compare above, as in the reference; its u, v must not become a map index: the reference reads out of bounds there)
    if (om.map && (u != u || v != v || !omm_opaque(om, prim, u, v))) return false;
    h.t = t; h.u = u; h.v = v;
    return true;
}

// Put right after the three loads of a triangle record: all three go out together.  Left alone the compiler sinks the third (v0, first needed behind
// the determinant test) into that branch — one load fewer for an edge-on triangle, a second memory round trip for every other one.
__device__ __forceinline__ void tri_loads_together(const float4& v0) { asm volatile("" :: "v"(v0.x), "v"(v0.y), "v"(v0.z), "v"(v0.w)); }

// Ballots of a bool straight from the compare that made it (HIP's __ballot takes an int: bool -> 0 / 1 -> compare again, two vector instructions
// per ballot), and lane counts as 32-bit SCALARS (the 64-bit value __popcll returns is compared with vector instructions: the scalar unit has no
// 64-bit ordered compare).
__device__ __forceinline__ unsigned long long wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ uint32_t wave_count(bool p) {
    const unsigned long long m = wave_ballot(p);
    uint32_t n;
    asm("s_bcnt1_i32_b64 %0, %1" : "=s"(n) : "s"(m) : "scc");
    return n;
}

__device__ __forceinline__ float3 xyz(float4 v) { return make_float3(v.x, v.y, v.z); }

// The library's tie rule.  tri_test has established t <= best.x; the candidate replaces the closest hit so far iff it is the
// first hit of this traversal, strictly closer, or equally far with the smaller primitive index (two-level kernels: then the smaller
// instance).  Every candidate at the final distance is tested whatever the visit order (nodes at tmin == best are visited: inclusive slab
// test), so the reported triangle does not depend on the schedule, on split rays or on the layout's child order.  The reference lets the
// LATER test win (tiny_bvh.h:1656: t <= ray.hit.t is accepted), i.e. its result among exactly equal t depends on the traversal order, and
// its own layouts disagree with each other there; oracle/tbvh_oracle.c restates both rules (orc_set_tie_rule).
// Box tests cull against a bound 2^-20 (eight ulps) beyond the closest hit so far.  A triangle lying IN a face of its leaf box — every
// axis-aligned wall — has its distance computed twice, by the slab test and by the triangle test, and the two round differently: with the
// exact bound, whether such a triangle is still tested once a hit within an ulp or two of it has been found depends on which was found
// first, i.e. on the traversal order (in the reference as well: tests/test_full_size.py).  With the slack every candidate within a few ulps of
// the closest hit is tested and the tie rule below picks the same one whatever the order; tri_test still rejects t > hit.t exactly, so no
// record gets farther, and a record can only get CLOSER (by ulps) than one the exact bound would have produced.
__device__ __forceinline__ float cull_bound(float t) { return t * 1.00000095367431640625f; }

__device__ __forceinline__ bool hit_wins(float t, uint32_t prim, bool found, float4 best) {
    return !found || t < best.x || prim < as_u32(best.w);
}
__device__ __forceinline__ bool hit_wins(float t, uint32_t prim, uint32_t inst, bool found, float4 best, uint32_t bestInst) {
    return !found || t < best.x || prim < as_u32(best.w) || (prim == as_u32(best.w) && inst < bestInst);
}

// The same rule for BVH_Double scenes (kernels_double.hip): the slack of the box culls is again eight ulps, 2^-49 in double, and a
// candidate that the triangle step has accepted against the closest hit so far replaces it iff it is strictly closer or, at EQUAL distance, a hit
// has been found already and the candidate has the smaller primitive index, then the smaller instance.  The reference's own test is strict
// (t < ray.hit.t, tiny_bvh.h:8194): the ray's tmax itself is never a hit, and among equal distances the FIRST found stays.
__device__ __host__ __forceinline__ double cull_bound_dbl(double t) { return t * 1.0000000000000017763568394002504646778106689453125; }
__device__ __host__ __forceinline__ bool hit_wins_dbl(double t, uint64_t prim, uint64_t inst, bool found, double bestT, uint64_t bestPrim, uint64_t bestInst) {
    return t < bestT || (found && t == bestT && (prim < bestPrim || (prim == bestPrim && inst < bestInst)));
}

// Kernel launch parameters common to the query kernels.
struct QueryArgs {
    RayRec* rays;          // device, 64-byte stride
    uint64_t nRays;
    uint8_t* occluded;     // any-hit output (1 byte per ray) or nullptr
    uint32_t* spill;       // global overflow area for traversal stacks
    uint32_t spillStride;  // entries per lane in `spill`
    uint32_t* counter;     // dynamic ray-fetch counters (persistent kernels): poolParts of them, 256 bytes apart
    uint32_t* counterNext; // the counter area of the next launch on this context: zeroed by this one (ray_pool.h: RayPool::init); nullptr: no
    uint32_t poolParts;    // log2 of the number of partitions of the batch, each with its own counter (ray_pool.h)
    // A scene in watertight mode (tbvh_set_triangle_test) hands its kernels two more words — its vertices, 3 float4 per triangle in primitive order, fetched
    // through a record's primitive index (v0 + e1 is not v1), and their count: a primitive index >= wtTris is never used as an address.  They SHARE the
    // storage of two members no watertight instantiation reads (it is never instrumented and never walks the hybrid node copy), so that the struct, and with
    // it the argument layout and the code of every other kernel, is what it was.  capi_query.hip sets them last, on the copy it launches with.
    union {
        unsigned long long* stats;  // instrumented variants: lane-utilisation counters
        const float4* wtVerts;      // watertight instantiations (kernels_cwbvh.hip: WT)
    };
    const unsigned long long* nRaysDev;  // if non-null the batch size is read from device memory (on-device queues)
    uint64_t splitBelow;   // batches of fewer rays split their last rays over idle lanes (ray_split.h); 0: never (TBVH_SPLIT_RAYS=0)
    Omm omm;               // opacity micromaps of the scene (map == nullptr: none)
    uint32_t fresh;        // 1: ignore the stored hit, start every ray from {freshTmax,0,0,0} and always write the record
    float freshTmax;
    // coherence probe of this batch (kernels_cwbvh.hip: coherence_sample, run by the traversal kernel itself): probe[0] = sampled neighbour pairs whose
    // directions agree, probe[1] = pairs sampled (published by the first kernel of the query); nullptr = this launch does not probe (small batches).
    // baseBlocks: workgroups beyond this index only take part when the batch is coherent.
    uint32_t* probe;
    uint32_t baseBlocks;
    uint32_t flags;        // 1 = non-temporal ray loads / hit stores, 2 = triangle records padded to 64 bytes (experiments); 16 = take the batch for coherent whatever the probe finds (variant 91); 32 = the first kernel of a two-flavor launch runs the strict schedule (PROBED == 4)
    union {
        uint32_t hybridK;  // BVH8_CWBVH, hybrid node array (cwbvh_node.h: kNodeHybrid): nodes below this index are packed, the others one per line
        uint32_t wtTris;   // watertight instantiations: triangles in wtVerts
    };
    // the same two probe counts once more, for the host: two words of host-coherent pinned memory that the kernel publishing `probe` also stores
    // (cwbvh_probe.h: probe_publish); nullptr: nobody remembers this launch's verdict.  flags & 64: the launch is the incoherent flavor ALONE (capi_query.hip:
    // a buffer whose last launches were incoherent) — its block 0 takes the sample and publishes it, no wave acts on it.
    uint32_t* probeHost = nullptr;
};
constexpr uint32_t kStatusWatertightPrim = 2048u;   // status word: a triangle record of a watertight scene names a primitive beyond the vertices it was given

// Host side: does this launch use the kernels with split rays?  Batches below the threshold, and the wavefront stages (ray count
// known to the device only); at 16.7 M rays the tail is 5 % of a launch and those kernels' register cap costs as much as it gains.
inline bool split_rays_wanted(const QueryArgs& q) { return q.splitBelow != 0 && (q.nRaysDev != nullptr || q.nRays < q.splitBelow); }


// A float4 array known to live in global memory.  Pointers that were themselves loaded from
// memory (per-BLAS node / triangle bases) are generic to the compiler, and loads through them
// become flat_load: same latency, but they also hold lgkmcnt, so LDS stack traffic and node
// fetches serialise.  GlobalF4 carries the address space, so the loads stay global_load.
typedef float tbvh_f4 __attribute__((ext_vector_type(4)));
struct GlobalF4 {
    const __attribute__((address_space(1))) tbvh_f4* p;
    __device__ __forceinline__ GlobalF4() : p(nullptr) {}
    __device__ __forceinline__ explicit GlobalF4(const float4* q) : p((const __attribute__((address_space(1))) tbvh_f4*)q) {}
    __device__ __forceinline__ float4 operator[](size_t i) const { const tbvh_f4 v = p[i]; return make_float4(v.x, v.y, v.z, v.w); }
    __device__ __forceinline__ GlobalF4 operator+(size_t o) const { GlobalF4 r; r.p = p + o; return r; }
};

}  // namespace tbvh
