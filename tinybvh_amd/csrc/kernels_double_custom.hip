// kernels_double_custom.hip — BVH_Double over custom geometry (spheres) for gfx950 (MI355X), in fp64: the sphere forms of k_double
// (kernels_double.hip), closest / any hit x BLAS / TLAS, and the record gather of an upload.
//
// The traversal is k_double's, statement for statement: persistent one-wave workgroups, per-lane ray replacement (ray_pool.h), the stack top in
// LDS and the rest in the spill area (lane_stack.h; overflow is reported as TBVH_E_FORMAT), blasBase in a register, one node visit or one primitive
// test per lane per iteration, the box test and the culls of double_step.h.  What differs:
//   - a BLAS's leaf holds sphere records (custom_sphere_dbl.h: the test, the winner rule, the deviation for occlusion), 48 bytes each;
//   - under a TLAS each BLAS is triangles or spheres: the low bit of its descriptor's record pointer says which (records are 16-byte aligned; the
//     bit is set by tbvh_upload_tlas_double only in a TLAS that has a sphere BLAS, and only such a TLAS is traced here: k_double never sees it);
//   - the per-ray factors of the sphere test (1 / |D|, tmax_in |D|) are computed once per ray, under a TLAS once per sphere instance from the
//     transformed D, against the record's INCOMING hit.t;
//   - a sphere hit leaves u, v of the record alone: they are written only when a triangle is the winner.
//
// The device build of a sphere BLAS is kernels_double_anim.hip's LBVH with the spheres as its box source.
#include <hip/hip_runtime.h>

#include "custom_sphere_dbl.h"
#include "device_common.h"
#include "double_step.h"
#include "kernels.h"
#include "lane_stack.h"
#include "ray_pool.h"

namespace tbvh {

namespace {

constexpr int WG = 64;
constexpr int LDS_N = 16;
constexpr int REFILL_MIN = 16;

template <bool ANYHIT, bool TLAS>
__global__ __launch_bounds__(WG) void k_double_custom(DoubleArgs q, uint32_t* __restrict__ status) {
    __shared__ uint32_t stk[LDS_N][WG];
    LaneStack<uint32_t, LDS_N, WG> st;
    st.init(&stk[0][threadIdx.x], q.spill + (blockIdx.x * WG + threadIdx.x), (size_t)gridDim.x * WG, q.spillStride);
    RayPool<64> pool;
    pool.init(q.poolParts, q.counterNext);

    bool active = false, found = false, haveNode = false, inBlas = false;
    bool sphBlas = !TLAS;              // the BLAS being traversed holds spheres
    bool triWon = false;               // the closest hit so far is a triangle's: u, v go back with it
    uint64_t ri = 0;
    D3 O{0, 0, 0}, D = O, rD = O;      // the ray being traversed (object space inside a BLAS)
    D3 wO = O, wD = O, wrD = O;        // TLAS: the world-space ray
    double ht = 0, hu = 0, hv = 0, tIn = 0;
    SphereRayDbl sr{0, 0};
    uint64_t hprim = 0, hinst = 0, rayInst = 0, rayMask = 0, curInst = 0;
    uint32_t node = 0;
    int blasBase = 0;                  // TLAS: stack height at which the current BLAS traversal began
    uint64_t primLeft = 0, primPtr = 0, instLeft = 0, instPtr = 0;
    const NodeDbl* nodes = q.nodes;
    const TriDbl* recs = q.tris;       // triangle records, or sphere records (sphBlas)

    for (;;) {
        const uint32_t nIdle = wave_count(!active);
        if (nIdle >= (uint32_t)REFILL_MIN) {
            if (!pool.dry()) {
                uint64_t nri = 0;
                if (pool.acquire(!active, q.counter, q.nRays, nri)) {
                    ri = nri;
                    const double2* r = (const double2*)(q.rays + ri);
                    const double2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4], r7 = r[7];
                    O = D3{r0.x, r0.y, r1.x}; D = D3{r1.y, r2.x, r2.y}; rD = D3{r3.x, r3.y, r4.x};
                    ht = r4.y; tIn = ht;
                    rayInst = __double_as_longlong(r7.x); rayMask = __double_as_longlong(r7.y);
                    wO = O; wD = D; wrD = rD;
                    if (!TLAS) sr = sphere_ray_dbl(D.x, D.y, D.z, tIn);
                    found = false; triWon = false; haveNode = true; inBlas = false; node = 0; primLeft = 0; instLeft = 0; st.sp = 0;
                    nodes = q.nodes; recs = q.tris;
                    active = true;
                }
            }
            if (wave_ballot(active) == 0) break;
        }
        if (!active) continue;

        bool done = false;
        if (primLeft != 0 && sphBlas) {
            // ---- one sphere (custom_sphere_dbl.h) ----
            const double2* s = (const double2*)((const SphereRecDbl*)recs + primPtr);
            const double2 s0 = s[0], s1 = s[1], s2 = s[2];
            primPtr++; primLeft--;
            const uint64_t prim = (uint64_t)__double_as_longlong(s2.x);
            double stored;
            if (sphere_test_dbl(O.x, O.y, O.z, D.x, D.y, D.z, s0.x, s0.y, s1.x, s1.y, sr, stored)) {
                const uint64_t inst = TLAS ? curInst : rayInst;
                if (ANYHIT) { found = true; done = true; }
                else if (sphere_wins_dbl(stored, prim, inst, found, ht, hprim, hinst)) {
                    found = true; triWon = false; ht = stored; hprim = prim; hinst = inst;
                }
            }
        } else if (TLAS && primLeft != 0) {
            // ---- one triangle of a triangle BLAS (tiny_bvh.h:8177-8201, 8302-8316) ----
            double t, u, v;
            uint64_t prim;
            const bool in = tri_test_dbl((const double2*)(recs + primPtr), O, D, t, u, v, prim);
            primPtr++; primLeft--;
            if (in) {
                if (ANYHIT) {
                    if (t > 0 && t < ht) { found = true; done = true; }
                } else if (t > 0 && hit_wins_dbl(t, prim, curInst, found, ht, hprim, hinst)) {
                    found = true; triWon = true; ht = t; hu = u; hv = v; hprim = prim; hinst = curInst;
                }
            }
        } else if (TLAS && !inBlas && instLeft != 0) {
            // ---- one instance of a TLAS leaf: into its BLAS (tiny_bvh.h:8223-8238, 8326-8342) ----
            const uint64_t ii = q.tlasIdx[instPtr];
            instPtr++; instLeft--;
            const InstanceDbl* in = q.inst + ii;
            if (in->mask & rayMask) {
                const double* T = in->invTransform;
                O = xform_point(wO, T);
                D = xform_vector(wD, T);
                if (ANYHIT) rD = D3{guarded_rcp(D.x), guarded_rcp(D.y), guarded_rcp(D.z)};
                else rD = D3{1.0 / D.x, 1.0 / D.y, 1.0 / D.z};
                const BlasDbl b = q.blas[in->blasIdx];
                const uintptr_t rp = (uintptr_t)b.tris;
                nodes = b.nodes; recs = (const TriDbl*)(rp & ~(uintptr_t)1);
                sphBlas = (rp & 1) != 0;
                if (sphBlas) sr = sphere_ray_dbl(D.x, D.y, D.z, tIn);
                curInst = ii;
                blasBase = st.sp;
                inBlas = true; node = 0; haveNode = true;
            }
        } else if (haveNode) {
            // ---- one node: a leaf's range, or the two children's slab tests (tiny_bvh.h:8202-8214) ----
            const double2* n = (const double2*)(nodes + node);
            const double2 n3 = n[3];
            const uint64_t first = (uint64_t)__double_as_longlong(n3.x), cnt = (uint64_t)__double_as_longlong(n3.y);
            if (cnt != 0) {
                if (!TLAS || inBlas) { primPtr = first; primLeft = cnt; }
                else { instPtr = first; instLeft = cnt; }
                haveNode = false;
            } else {
                const double bound = cull_bound_dbl(ht);
                uint32_t c1 = (uint32_t)first, c2 = (uint32_t)first + 1u;
                double d1 = node_dist((const double2*)(nodes + c1), O, rD, bound), d2 = node_dist((const double2*)(nodes + c2), O, rD, bound);
                if (d1 > d2) { const double td = d1; d1 = d2; d2 = td; const uint32_t tc = c1; c1 = c2; c2 = tc; }
                if (d1 == kDblFar) haveNode = false;
                else {
                    node = c1;
                    if (d2 != kDblFar) st.push(c2);
                }
            }
        } else {
            // ---- pop: the end of a BLAS (back to the world ray and the rest of the TLAS leaf), the next node, or the end of the ray ----
            if (TLAS && inBlas && st.sp == blasBase) { O = wO; D = wD; rD = wrD; nodes = q.nodes; recs = q.tris; inBlas = false; }
            else if (st.sp == 0) done = true;
            else { node = st.pop(); haveNode = true; }
        }
        if (done) {
            if (ANYHIT) q.occluded[ri] = found ? 1 : 0;
            else if (found) {
                double2* r = (double2*)(q.rays + ri);
                r[4].y = ht;   // (r[4].x is rD.z)
                if (TLAS && triWon) r[5] = make_double2(hu, hv);
                r[6] = make_double2(__longlong_as_double((long long)hinst), __longlong_as_double((long long)hprim));
            }
            active = false;
        }
    }
    if (st.overflow) atomicOr(status, 1u);
}

// upload helper: {pos, r, prim, 0} per primIdx entry
__global__ void k_gather_spheres_dbl(const uint64_t* __restrict__ primIdx, const SphereDbl* __restrict__ sph, SphereRecDbl* __restrict__ out, uint64_t nIdx) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nIdx) return;
    const uint64_t p = primIdx[i];   // (< n_spheres: validated at upload)
    const SphereDbl s = sph[p];
    out[i] = SphereRecDbl{{s.pos[0], s.pos[1], s.pos[2]}, s.r, p, 0};
}

}  // namespace

void launch_double_custom(bool anyhit, bool tlas, const DoubleArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s) {
    if (tlas) {
        if (anyhit) hipLaunchKernelGGL((k_double_custom<true, true>), dim3(blocks), dim3(WG), 0, s, q, status);
        else hipLaunchKernelGGL((k_double_custom<false, true>), dim3(blocks), dim3(WG), 0, s, q, status);
    } else {
        if (anyhit) hipLaunchKernelGGL((k_double_custom<true, false>), dim3(blocks), dim3(WG), 0, s, q, status);
        else hipLaunchKernelGGL((k_double_custom<false, false>), dim3(blocks), dim3(WG), 0, s, q, status);
    }
}

void launch_gather_spheres_dbl(const uint64_t* primIdx, const void* spheres32, void* recs48, uint64_t nIdx, hipStream_t s) {
    const uint32_t bs = 256;
    hipLaunchKernelGGL(k_gather_spheres_dbl, dim3((uint32_t)((nIdx + bs - 1) / bs)), dim3(bs), 0, s, primIdx, (const SphereDbl*)spheres32, (SphereRecDbl*)recs48, nIdx);
}

}  // namespace tbvh
