// kernels_custom.hip — custom-geometry sphere BLASes on gfx950: BVH::Intersect / IsOccluded over a BVH built with BVH::Build( customGetAABB, n ),
// its custom branch (tiny_bvh.h:3270-3279, 3424-3428) with the sphere callback of the reference's anim demo (custom_sphere.h).
//
// Walk: the reference's — the root is entered without a box test, a node's two children are slab-tested together (SLAB_TEST_TWO_NODES, the near
// one first, the far one pushed), a leaf tests its spheres in primIdx order — with the library's rules: box culls against cull_bound(hit.t), and
// the winner is the candidate with the smallest recorded distance, then the smaller primitive (custom_sphere.h: sphere_wins), whatever the
// order the spheres are met in.  u and v are never written (the callback does not touch them); a hit writes t, prim and hit.inst = ray.instIdx.
//
// Structure: persistent one-wave workgroups, one lane = one ray, per-lane refill from a wave-local pool (ray_pool.h), per-lane stack of 8-byte
// entries {leftFirst, triCount} of the nodes still to visit, its top in LDS and a global spill area (lane_stack.h).  One iteration = one node
// visit (the sibling pair: one 64-byte read) or one sphere test per lane.
#include "device_common.h"
#include "custom_sphere.h"
#include "lane_stack.h"
#include "ray_pool.h"
#include "kernels.h"

namespace tbvh {

namespace {

constexpr int WG = 64;
constexpr int kCustomLds = 16;        // stack entries per lane in LDS (16 x 8 bytes x 64 lanes = 8 KB per wave)
constexpr uint32_t kRefillMin = 16;   // idle lanes that trigger a refill from the pool

typedef LaneStack<uint2, kCustomLds, WG> Stack64;

template <bool ANYHIT>
__global__ __launch_bounds__(WG) void k_custom(const float4* __restrict__ nodes, const float4* __restrict__ recs, const QueryArgs q,
                                               uint32_t* __restrict__ status) {
    __shared__ uint2 stk[kCustomLds][WG];
    Stack64 st;
    st.init(&stk[0][threadIdx.x], (uint2*)q.spill + (blockIdx.x * WG + threadIdx.x), (size_t)gridDim.x * WG, q.spillStride);
    RayPool<64> pool;
    pool.init(q.poolParts, q.counterNext);
    const uint64_t nRaysTotal = q.nRaysDev ? *q.nRaysDev : q.nRays;
    // the root's own leftFirst / triCount: every ray starts there
    const uint32_t rootFirst = as_u32(nodes[0].w), rootCount = as_u32(nodes[1].w);

    bool active = false, found = false;
    uint64_t ri = 0;
    float3 O = make_float3(0.f, 0.f, 0.f), D = O, rD = O, ro = O;
    bool px = true, py = true, pz = true;
    float4 hit = make_float4(0.f, 0.f, 0.f, 0.f);
    SphereRay sr{0.f, 0.f};
    uint32_t node = 0, leafPtr = 0, leafLeft = 0;

    for (;;) {
        const uint32_t nIdle = (uint32_t)__popcll(__ballot(!active));
        if (nIdle >= kRefillMin || nIdle == (uint32_t)WG) {
            if (!pool.dry()) {
                uint64_t nri = 0;
                if (pool.acquire(!active, q.counter, nRaysTotal, nri)) {
                    ri = nri;
                    const RayRec* rp = q.rays + ri;
                    O = xyz(rp->O); D = xyz(rp->D); rD = xyz(rp->rD);
                    hit = q.fresh ? make_float4(q.freshTmax, 0.f, 0.f, 0.f) : rp->hit;
                    px = D.x >= 0.f; py = D.y >= 0.f; pz = D.z >= 0.f;
                    ro = make_float3(O.x * rD.x, O.y * rD.y, O.z * rD.z);
                    sr = sphere_ray(D, hit.x);
                    found = false;
                    st.reset();
                    if (rootCount) { leafPtr = rootFirst; leafLeft = rootCount; }   // a one-leaf tree
                    else { node = rootFirst; leafLeft = 0; }
                    active = true;
                }
            }
            if (__ballot(active) == 0) break;
        }
        if (!active) continue;

        bool done = false, pop = false;
        if (leafLeft != 0) {   // ---- one sphere ---------------------------------------------------------------------------------------------
            const float4 s = recs[(size_t)leafPtr * 2], pr = recs[(size_t)leafPtr * 2 + 1];
            leafPtr++; leafLeft--;
            float t;
            if (sphere_test(O, D, s, sr, t)) {
                const uint32_t prim = as_u32(pr.x);
                if (ANYHIT) { found = true; done = true; }
                else if (sphere_wins(t, prim, 0u, found, hit, 0u)) { hit.x = t; hit.w = as_f32(prim); found = true; }
            }
            if (!done && leafLeft == 0) pop = true;
        } else {               // ---- one node: its two children ------------------------------------------------------------------------------
            const float4 a0 = nodes[(size_t)node * 2], a1 = nodes[(size_t)node * 2 + 1], b0 = nodes[(size_t)node * 2 + 2], b1 = nodes[(size_t)node * 2 + 3];
            const float bound = cull_bound(hit.x);
            float d1 = wald_slab(a0, a1, rD, ro, px, py, pz, bound), d2 = wald_slab(b0, b1, rD, ro, px, py, pz, bound);
            uint2 c1 = make_uint2(as_u32(a0.w), as_u32(a1.w)), c2 = make_uint2(as_u32(b0.w), as_u32(b1.w));
            if (d1 > d2) { const float tf = d1; d1 = d2; d2 = tf; const uint2 tc = c1; c1 = c2; c2 = tc; }
            if (d1 == kFar) pop = true;
            else {
                if (d2 != kFar) st.push(c2);
                if (c1.y) { leafPtr = c1.x; leafLeft = c1.y; } else node = c1.x;
            }
        }
        if (pop) {
            if (st.empty()) done = true;
            else {
                const uint2 e = st.pop();
                if (e.y) { leafPtr = e.x; leafLeft = e.y; } else node = e.x;
            }
        }
        if (done) {
            RayRec* rp = q.rays + ri;
            if (ANYHIT) q.occluded[ri] = found ? 1 : 0;
            else if (found) { rp->hit = hit; ((uint32_t*)rp)[11] = as_u32(rp->D.w); }   // byte 44 = hit.inst = ray.instIdx (tiny_bvh.h:3274-3275)
            else if (q.fresh) rp->hit = hit;
            active = false;
        }
    }
    if (st.overflow) atomicOr(status, 1u);
}

}  // namespace

void launch_custom(bool anyhit, const float4* nodes, const float4* recs, const QueryArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s) {
    if (anyhit) hipLaunchKernelGGL(k_custom<true>, dim3(blocks), dim3(WG), 0, s, nodes, recs, q, status);
    else hipLaunchKernelGGL(k_custom<false>, dim3(blocks), dim3(WG), 0, s, nodes, recs, q, status);
}

}  // namespace tbvh
