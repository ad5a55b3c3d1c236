// kernels_sphere.hip — BVH::IntersectSphere (tiny_bvh.h:3140-3200) batched on gfx950: does sphere i = {x, y, z, r} touch any triangle?
// One any-hit traversal per BLAS layout (BVH_GPU, BVH4_GPU, BVH8_CWBVH), over the uploaded node arrays; the triangle test reads the
// caller's vertex array (3 bvhvec4 per triangle) at the primitive index the layout's triangle record carries.
//
// Arithmetic (DESIGN.md par. 11): the reference's operations in its order, with the products GCC fuses in the x86 build of oracle/Makefile
// (-O3 -mavx2 -mfma; read from the disassembly of BVH::IntersectSphere) written as explicit fmas — the library builds with
// -ffp-contract=off, so nothing else is fused.  tests/oracle_sphere.c restates the same operations; the device matches it byte for byte.
//   dist2 += d * d                     fma(d, d, dist2)
//   cross(u, v).x = u.y v.z - u.z v.y   fma(u.y, v.z, -(u.z v.y))   (and cyclically)
//   dot(p, q)                          fma(p.z, q.z, fma(p.x, q.x, p.y q.y)) — except e3 = dot(CA, CA): fma(z, z, fma(y, y, x x))
//   Q1 = A e1 - AB d1, Q2 = B e2 - BC d2     fma(-AB, d1, A e1), fma(-BC, d2, B e2)
//   Q3 = C e3 - CA d3                  fma(C, e3, -(CA d3))
//   QC = C e1 - Q1, QA = A e2 - Q2, QB = B e3 - Q3     fma(C, e1, -Q1) ...
// Walk: the reference's tests — a child is entered if its box overlaps the sphere's box strictly, a leaf's triangles are tested only if the
// squared distance from the centre to the leaf's box is <= r^2 — with one deliberate deviation: a node taken off the stack goes through the
// leaf check (the reference treats it as an interior node: defect 1 of DESIGN.md par. 11).  BVH_GPU child boxes are the Wald BVH's bit for
// bit; the 4- and 8-wide layouts use their quantised child boxes as written.
//
// Structure: persistent one-wave workgroups, one lane = one sphere, per-lane refill from a wave-local pool (ray_pool.h), per-lane stack of
// 8-byte entries with its top in LDS and a global spill area (lane_stack.h).  An entry is a node {address, 0} or a leaf {first record,
// count}; BVH_GPU entries are nodes whose leafness is known only once fetched, so they carry the leaf test's verdict instead: {node, 1}
// when the box failed the distance test.  One iteration = at most one pop (node visit or leaf start) and one triangle test per lane.
#include "device_common.h"
#include "mesh_source.h"
#include "cwbvh_node.h"
#include "lane_stack.h"
#include "ray_pool.h"
#include "kernels.h"

namespace tbvh {

namespace {

constexpr int WG = 64;
constexpr int kSphereLds = 16;        // stack entries per lane in LDS (16 x 8 bytes x 64 lanes = 8 KB per wave)
constexpr uint32_t kRefillMin = 16;   // idle lanes that trigger a refill from the pool

typedef LaneStack<uint2, kSphereLds, WG> Stack64;

struct Sphere {
    float3 pos, bmin, bmax;
    float r, r2;
};

// BVHNode::Intersect( bmin, bmax ) (tiny_bvh.h:8606-8611): strict on every face
__device__ __forceinline__ bool box_overlap(const Sphere& s, float3 mn, float3 mx) {
    return s.bmin.x < mx.x && s.bmax.x > mn.x && s.bmin.y < mx.y && s.bmax.y > mn.y && s.bmin.z < mx.z && s.bmax.z > mn.z;
}

// the leaf test of tiny_bvh.h:3150-3157: squared distance from the centre to the box, x, y, z in that order
__device__ __forceinline__ bool leaf_near(const Sphere& s, float3 mn, float3 mx) {
    float dist2 = 0.f;
    if (s.pos.x < mn.x) { const float d = mn.x - s.pos.x; dist2 = __fmaf_rn(d, d, dist2); }
    if (s.pos.x > mx.x) { const float d = s.pos.x - mx.x; dist2 = __fmaf_rn(d, d, dist2); }
    if (s.pos.y < mn.y) { const float d = mn.y - s.pos.y; dist2 = __fmaf_rn(d, d, dist2); }
    if (s.pos.y > mx.y) { const float d = s.pos.y - mx.y; dist2 = __fmaf_rn(d, d, dist2); }
    if (s.pos.z < mn.z) { const float d = mn.z - s.pos.z; dist2 = __fmaf_rn(d, d, dist2); }
    if (s.pos.z > mx.z) { const float d = s.pos.z - mx.z; dist2 = __fmaf_rn(d, d, dist2); }
    return dist2 <= s.r2;
}

__device__ __forceinline__ float3 sub3(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float dot_yxz(float3 p, float3 q) { return __fmaf_rn(p.z, q.z, __fmaf_rn(p.x, q.x, p.y * q.y)); }
__device__ __forceinline__ float dot_xyz(float3 p, float3 q) { return __fmaf_rn(p.z, q.z, __fmaf_rn(p.y, q.y, p.x * q.x)); }

// the separating-axis sphere / triangle test of tiny_bvh.h:3160-3188 on the original vertices
__device__ __forceinline__ bool tri_sphere(const Sphere& s, float3 a, float3 b, float3 c) {
    const float3 A = sub3(a, s.pos), B = sub3(b, s.pos), C = sub3(c, s.pos);
    const float rr = s.r * s.r;
    const float3 u = sub3(B, A), v = sub3(C, A);
    const float3 V = make_float3(__fmaf_rn(u.y, v.z, -(u.z * v.y)), __fmaf_rn(u.z, v.x, -(u.x * v.z)), __fmaf_rn(u.x, v.y, -(u.y * v.x)));
    const float d = dot_yxz(A, V), e = dot_yxz(V, V);
    if (d * d > rr * e) return false;
    const float aa = dot_yxz(A, A), ab = dot_yxz(A, B), ac = dot_yxz(A, C);
    const float bb = dot_yxz(B, B), bc = dot_yxz(B, C), cc = dot_yxz(C, C);
    if ((aa > rr && ab > aa && ac > aa) || (bb > rr && ab > bb && bc > bb) || (cc > rr && ac > cc && bc > cc)) return false;
    const float3 AB = u, BC = sub3(C, B), CA = sub3(A, C);
    const float d1 = ab - aa, d2 = bc - bb, d3 = ac - cc;
    const float e1 = dot_yxz(AB, AB), e2 = dot_yxz(BC, BC), e3 = dot_xyz(CA, CA);
    const float3 Q1 = make_float3(__fmaf_rn(-AB.x, d1, A.x * e1), __fmaf_rn(-AB.y, d1, A.y * e1), __fmaf_rn(-AB.z, d1, A.z * e1));
    const float3 Q2 = make_float3(__fmaf_rn(-BC.x, d2, B.x * e2), __fmaf_rn(-BC.y, d2, B.y * e2), __fmaf_rn(-BC.z, d2, B.z * e2));
    const float3 Q3 = make_float3(__fmaf_rn(C.x, e3, -(CA.x * d3)), __fmaf_rn(C.y, e3, -(CA.y * d3)), __fmaf_rn(C.z, e3, -(CA.z * d3)));
    const float3 QC = make_float3(__fmaf_rn(C.x, e1, -Q1.x), __fmaf_rn(C.y, e1, -Q1.y), __fmaf_rn(C.z, e1, -Q1.z));
    const float3 QA = make_float3(__fmaf_rn(A.x, e2, -Q2.x), __fmaf_rn(A.y, e2, -Q2.y), __fmaf_rn(A.z, e2, -Q2.z));
    const float3 QB = make_float3(__fmaf_rn(B.x, e3, -Q3.x), __fmaf_rn(B.y, e3, -Q3.y), __fmaf_rn(B.z, e3, -Q3.z));
    if ((dot_yxz(Q1, Q1) > rr * e1 * e1 && dot_yxz(Q1, QC) >= 0.f) || (dot_yxz(Q2, Q2) > rr * e2 * e2 && dot_yxz(Q2, QA) >= 0.f) ||
        (dot_yxz(Q3, Q3) > rr * e3 * e3 && dot_yxz(Q3, QB) >= 0.f))
        return false;
    return true;
}

// the primitive index of a triangle record: BVH_GPU gathered {v0|prim, e1, e2} (k = primIdx entry), BVH4_GPU inline {v0|prim, e1, e2} and
// CWBVH {e2, e1, v0|prim} (k = the record's first float4: both layouts address triangles in float4s, tiny_bvh.h:5160-5166, 5999-6003)
template <int LAYOUT> __device__ __forceinline__ uint32_t record_prim(const float4* __restrict__ tris, uint32_t k) {
    if (LAYOUT == kLayoutBvh4Gpu) return as_u32(tris[k].w);
    if (LAYOUT == kLayoutCwbvh) return as_u32(tris[(size_t)k + 2].w);
    return as_u32(tris[(size_t)k * 3].w);
}

template <int LAYOUT, bool GENERAL>
__global__ __launch_bounds__(WG) void k_spheres(const SphereArgs q, uint32_t* __restrict__ status) {
    __shared__ uint2 stk[kSphereLds][WG];
    Stack64 st;
    st.init(&stk[0][threadIdx.x], (uint2*)q.spill + (blockIdx.x * WG + threadIdx.x), (size_t)gridDim.x * WG, q.spillStride);
    RayPool<64> pool;
    pool.init(q.poolParts, q.counterNext);
    const float4* __restrict__ nodes = q.nodes;
    const float4* __restrict__ tris = LAYOUT == kLayoutBvh4Gpu ? q.nodes : q.tris;
    const MeshSrc& verts = q.verts;   // the triangle test's vertices: mesh_source.h
    const uint64_t nTris = q.verts.nTris;

    bool active = false;
    uint64_t si = 0;
    Sphere s;
    s.pos = s.bmin = s.bmax = make_float3(0.f, 0.f, 0.f);
    s.r = s.r2 = 0.f;
    uint32_t triPtr = 0, triLeft = 0;   // the current leaf's records still to test (BVH4_GPU / CWBVH: float4 address, step 3)
    bool badPrim = false, badIndex = false;

    for (;;) {
        const uint32_t nIdle = (uint32_t)__popcll(__ballot(!active));
        if (nIdle >= kRefillMin || nIdle == (uint32_t)WG) {
            if (!pool.dry()) {
                uint64_t nsi = 0;
                if (pool.acquire(!active, q.counter, q.nSpheres, nsi)) {
                    si = nsi;
                    const float4 p = q.spheres[si];
                    s.pos = make_float3(p.x, p.y, p.z);
                    s.r = p.w;
                    s.bmin = make_float3(p.x - p.w, p.y - p.w, p.z - p.w);
                    s.bmax = make_float3(p.x + p.w, p.y + p.w, p.z + p.w);
                    s.r2 = p.w * p.w;
                    triLeft = 0;
                    st.reset();
                    st.push(make_uint2(0u, 0u));   // the root: never box-tested (a leaf root gets its distance test when fetched)
                    active = true;
                }
            }
            if (__ballot(active) == 0) break;
        }
        if (!active) continue;

        bool done = false, found = false;
        // ---- one pop: a node visit or the start of a leaf ----------------------------------------------------------------------
        if (triLeft == 0) {
            if (st.empty()) done = true;
            else {
                const uint2 e = st.pop();
                if (LAYOUT == kLayoutBvhGpu) {
                    const float4 n0 = nodes[(size_t)e.x * 4], n1 = nodes[(size_t)e.x * 4 + 1], n2 = nodes[(size_t)e.x * 4 + 2], n3 = nodes[(size_t)e.x * 4 + 3];
                    const uint32_t cnt = as_u32(n2.w);
                    if (cnt) {
                        bool near = e.y == 0u;
                        if (e.x == 0u) {   // a leaf root: its box, zero in this layout, is the min / max of its triangles' vertices
                            float3 mn = make_float3(kFar, kFar, kFar), mx = make_float3(-kFar, -kFar, -kFar);
                            for (uint32_t k = 0; k < cnt; k++) {
                                const uint32_t prim = record_prim<LAYOUT>(tris, as_u32(n3.w) + k);
                                if (prim >= nTris) { badPrim = true; continue; }
                                float4 tv[3];
                                if (!mesh_tri<GENERAL>(verts, prim, tv[0], tv[1], tv[2])) { badIndex = true; continue; }
                                for (int j = 0; j < 3; j++) {
                                    const float4 v = tv[j];
                                    mn = make_float3(fminf(mn.x, v.x), fminf(mn.y, v.y), fminf(mn.z, v.z));
                                    mx = make_float3(fmaxf(mx.x, v.x), fmaxf(mx.y, v.y), fmaxf(mx.z, v.z));
                                }
                            }
                            near = leaf_near(s, mn, mx);
                        }
                        if (near) { triPtr = as_u32(n3.w); triLeft = cnt; }
                    } else {
                        // n0 = lmin | left, n1 = lmax | right, n2 = rmin | triCount, n3 = rmax | firstTri
                        const float3 lmn = make_float3(n0.x, n0.y, n0.z), lmx = make_float3(n1.x, n1.y, n1.z);
                        const float3 rmn = make_float3(n2.x, n2.y, n2.z), rmx = make_float3(n3.x, n3.y, n3.z);
                        if (box_overlap(s, rmn, rmx)) st.push(make_uint2(as_u32(n1.w), leaf_near(s, rmn, rmx) ? 0u : 1u));
                        if (box_overlap(s, lmn, lmx)) st.push(make_uint2(as_u32(n0.w), leaf_near(s, lmn, lmx) ? 0u : 1u));
                    }
                } else if (e.y) {
                    triPtr = e.x; triLeft = e.y;
                } else if (LAYOUT == kLayoutBvh4Gpu) {
                    // d0 = bmin | qx0, d1 = (bmax - bmin) / 255 | qx1, d2 = qy0 qy1 qz0 qz1, d3 = child info (tiny_bvh.h:5115-5236)
                    const float4 d0 = nodes[e.x], d1 = nodes[e.x + 1], d2 = nodes[e.x + 2], d3 = nodes[e.x + 3];
                    const uint32_t qx0 = as_u32(d0.w), qx1 = as_u32(d1.w), qy0 = as_u32(d2.x), qy1 = as_u32(d2.y), qz0 = as_u32(d2.z), qz1 = as_u32(d2.w);
                    const uint32_t info[4] = {as_u32(d3.x), as_u32(d3.y), as_u32(d3.z), as_u32(d3.w)};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        if (info[i] == 0u) continue;
                        const int sh = 8 * i;
                        const float3 mn = make_float3(d0.x + (float)((qx0 >> sh) & 255u) * d1.x, d0.y + (float)((qy0 >> sh) & 255u) * d1.y, d0.z + (float)((qz0 >> sh) & 255u) * d1.z);
                        const float3 mx = make_float3(d0.x + (float)((qx1 >> sh) & 255u) * d1.x, d0.y + (float)((qy1 >> sh) & 255u) * d1.y, d0.z + (float)((qz1 >> sh) & 255u) * d1.z);
                        if (!box_overlap(s, mn, mx)) continue;
                        if (info[i] & 0x80000000u) {
                            const uint32_t cnt = (info[i] >> 16) & 0x7fffu;
                            if (cnt && leaf_near(s, mn, mx)) st.push(make_uint2(e.x + (info[i] & 0xffffu), cnt));
                        } else st.push(make_uint2(info[i], 0u));
                    }
                } else {
                    // n0 = origin | ex ey ez imask, n1 = child base | triangle base | meta[8], n2-n4 = quantised planes (cwbvh_node.h)
                    const CwNode nr = CwNode{nodes[(size_t)e.x * 5], nodes[(size_t)e.x * 5 + 1], nodes[(size_t)e.x * 5 + 2], nodes[(size_t)e.x * 5 + 3], nodes[(size_t)e.x * 5 + 4]};
                    const uint32_t ew = as_u32(nr.n0.w), imask = ew >> 24;
                    const float sx = ldexpf(1.f, (int)(int8_t)(ew)), sy = ldexpf(1.f, (int)(int8_t)(ew >> 8)), sz = ldexpf(1.f, (int)(int8_t)(ew >> 16));
                    const uint32_t childBase = as_u32(nr.n1.x), triBase = as_u32(nr.n1.y);
#pragma unroll
                    for (int half = 0; half < 2; half++) {
                        const uint32_t meta4 = half ? as_u32(nr.n1.w) : as_u32(nr.n1.z);
                        const uint32_t qlx = half ? as_u32(nr.n2.y) : as_u32(nr.n2.x), qhx = half ? as_u32(nr.n3.w) : as_u32(nr.n3.z);
                        const uint32_t qly = half ? as_u32(nr.n2.w) : as_u32(nr.n2.z), qhy = half ? as_u32(nr.n4.y) : as_u32(nr.n4.x);
                        const uint32_t qlz = half ? as_u32(nr.n3.y) : as_u32(nr.n3.x), qhz = half ? as_u32(nr.n4.w) : as_u32(nr.n4.z);
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int sh = 8 * i, slot = 4 * half + i;
                            const uint32_t meta = (meta4 >> sh) & 255u;
                            if (meta == 0u) continue;
                            const float3 mn = make_float3(nr.n0.x + (float)((qlx >> sh) & 255u) * sx, nr.n0.y + (float)((qly >> sh) & 255u) * sy, nr.n0.z + (float)((qlz >> sh) & 255u) * sz);
                            const float3 mx = make_float3(nr.n0.x + (float)((qhx >> sh) & 255u) * sx, nr.n0.y + (float)((qhy >> sh) & 255u) * sy, nr.n0.z + (float)((qhz >> sh) & 255u) * sz);
                            if (!box_overlap(s, mn, mx)) continue;
                            if (imask & (1u << slot)) st.push(make_uint2(childBase + (uint32_t)__popc(imask & ((1u << slot) - 1u)), 0u));
                            else if (leaf_near(s, mn, mx)) st.push(make_uint2(triBase + 3u * (meta & 31u), (uint32_t)__popc((meta >> 5) & 7u)));
                        }
                    }
                }
            }
        }
        // ---- one triangle ---------------------------------------------------------------------------------------------------------
        if (triLeft != 0 && !done) {
            const uint32_t prim = record_prim<LAYOUT>(tris, triPtr);
            triPtr += LAYOUT == kLayoutBvhGpu ? 1u : 3u; triLeft--;
            float4 a, b, c;
            if (prim >= nTris) badPrim = true;   // (a vertex array shorter than the blob: tbvh_intersect_spheres reports it)
            else if (!mesh_tri<GENERAL>(verts, prim, a, b, c)) badIndex = true;   // (an index beyond the vertices: never dereferenced)
            else {
                if (tri_sphere(s, make_float3(a.x, a.y, a.z), make_float3(b.x, b.y, b.z), make_float3(c.x, c.y, c.z))) { found = true; done = true; }
            }
            if (!done && triLeft == 0 && st.empty()) done = true;
        }
        if (done) {
            q.hit[si] = found ? 1 : 0;
            active = false;
        }
    }
    if (st.overflow) atomicOr(status, 1u);
    if (badPrim) atomicOr(status, 16u);
    if (GENERAL && badIndex) atomicOr(status, kStatusMeshIndex);
}

}  // namespace

void launch_spheres(int layout, const SphereArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s) {
#define TBVH_LS(L)                                                                                                    \
    do {                                                                                                              \
        if (q.verts.general()) hipLaunchKernelGGL((k_spheres<L, true>), dim3(blocks), dim3(WG), 0, s, q, status);     \
        else hipLaunchKernelGGL((k_spheres<L, false>), dim3(blocks), dim3(WG), 0, s, q, status);                      \
    } while (0)
    if (layout == kLayoutBvh4Gpu) TBVH_LS(kLayoutBvh4Gpu);
    else if (layout == kLayoutCwbvh) TBVH_LS(kLayoutCwbvh);
    else TBVH_LS(kLayoutBvhGpu);
#undef TBVH_LS
}

}  // namespace tbvh
