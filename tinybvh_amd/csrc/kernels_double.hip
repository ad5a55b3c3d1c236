// kernels_double.hip — BVH_Double Intersect / IsOccluded / IntersectTLAS / IsOccludedTLAS for gfx950 (MI355X), in fp64, over triangles and over
// custom geometry (spheres), and the record gathers of the two uploads.
//
// One traversal, eight instantiations (triangle records only / sphere records x closest / any hit x BLAS / TLAS), restating tiny_bvh.h:8158-8375
// rather than approximating it:
//   - BVHNode::Intersect (:8363-8375): (plane - O) * rD per slab, tinybvh_min / _max as the ternaries `a < b ? a : b` / `a > b ? a : b`
//     (:447-448), NOT fmin / v_min_f64: they differ where a product is NaN (origin on a slab plane, rD = inf), which is what the RayEx
//     constructor makes of every axis-parallel ray.  A child is visited iff tmax >= tmin && tmin < hit.t && tmax >= 0.
//   - the root is not box-tested; the nearer child is taken, the farther one pushed (dist1 > dist2 swaps); both missed: pop.
//   - Moller-Trumbore with the |a| < 1e-7 reject (:8177-8194); e1, e2 are precomputed at upload by the same double subtraction
//     (k_gather_tris_dbl), f = 1 / a is the correctly rounded division (hipcc default for double), and the Makefile's -ffp-contract=off
//     keeps every product and sum a separate IEEE operation, evaluated in the reference's order.
//   - TLAS (:8220-8266, 8318-8360): an instance is skipped unless inst.mask & ray.mask; the ray goes through invTransform with
//     tinybvh_transform_point / _vector (:576-590, the w != 1 divide included); rD = 1.0 / D unguarded for closest hits, guarded with
//     1e-24 -> BVH_DBL_FAR for any-hit queries; the BLAS is traversed completely before the next instance of the leaf.
//   - a hit needs t > 0 and wins by the library's rule (device_common.h: hit_wins_dbl, cull_bound_dbl): at equal t the smaller prim,
//     then the smaller instance; box culls allow eight ulps beyond the closest hit.  Occlusion: 0 < t < hit.t.
// The per-ray visit order is the reference's; only the stack is different: its top in LDS and the rest in the global spill area
// (lane_stack.h), so trees deeper than the reference's stack[64] work.  A TLAS ray keeps the stack height at which its current BLAS began
// (blasBase, as kernels_tlas2.hip does) instead of a marker entry: when the stack is full, LaneStack::push drops the entry and sets
// `overflow` (reported as TBVH_E_FORMAT), and a dropped marker would let the BLAS traversal pop TLAS entries as BLAS nodes.  With the
// height kept in a register, entries [0, blasBase) are TLAS nodes and [blasBase, sp) nodes of the current BLAS; a BLAS pops only while
// sp > blasBase, the TLAS only once the BLAS is left, so a popped index always belongs to the tree `nodes` points at, overflow or not.  Persistent one-wave workgroups with per-lane ray replacement
// (ray_pool.h), as in kernels_query.hip; one node visit or one primitive test per lane per iteration.
//
// SPH, the sphere forms (a sphere BLAS, or a TLAS that lists one).  The loop is the same; what differs, all of it compiled out of the
// triangle-only forms:
//   - a BLAS's leaf holds sphere records (custom_sphere_dbl.h: the test, the winner rule, the deviation for occlusion), 48 bytes each;
//   - under a TLAS each BLAS is triangles or spheres: the low bit of its descriptor's record pointer says which (records are 16-byte aligned; the
//     bit is set by tbvh_upload_tlas_double only in a TLAS that has a sphere BLAS, and only such a TLAS is traced by a sphere form: the
//     triangle-only forms read plain pointers);
//   - the per-ray factors of the sphere test (1 / |D|, tmax_in |D|) are computed once per ray, under a TLAS once per sphere instance from the
//     transformed D, against the record's INCOMING hit.t;
//   - a sphere hit leaves u, v of the record alone: they are written only when a triangle is the winner;
//   - the triangle step of a TLAS that lists a sphere BLAS is written through tri_test_dbl (double_step.h), that of the triangle-only forms inline.
//     The arithmetic is the same; the compiler's code is not, and neither spelling serves both: inline, the sphere TLAS forms sink the load of a
//     record's last 8 bytes into the hit block, wait at every join of the loop and trace 1.2-1.6 % slower (profiles/double_one_kernel.txt); through
//     the helper, each triangle-only form takes two more VGPRs.  With both, all eight forms are the code they were before the two kernels became one.
// The device build of a sphere BLAS is kernels_double_anim.hip's LBVH with the spheres as its box source.
#include "custom_sphere_dbl.h"
#include "device_common.h"
#include "double_step.h"
#include "lane_stack.h"
#include "ray_pool.h"
#include "kernels.h"

namespace tbvh {

namespace {

constexpr int WG = 64;
constexpr int LDS_N = 16;
constexpr int REFILL_MIN = 16;

template <bool SPH, bool ANYHIT, bool TLAS>
__global__ __launch_bounds__(WG) void k_double(DoubleArgs q, uint32_t* __restrict__ status) {
    __shared__ uint32_t stk[LDS_N][WG];
    LaneStack<uint32_t, LDS_N, WG> st;
    st.init(&stk[0][threadIdx.x], q.spill + (blockIdx.x * WG + threadIdx.x), (size_t)gridDim.x * WG, q.spillStride);
    RayPool<64> pool;
    pool.init(q.poolParts, q.counterNext);

    bool active = false, found = false, haveNode = false, inBlas = false;
    bool sphBlas = SPH && !TLAS;       // SPH: the BLAS being traversed holds spheres
    bool triWon = false;               // SPH: the closest hit so far is a triangle's: u, v go back with it
    uint64_t ri = 0;
    D3 O{0, 0, 0}, D = O, rD = O;      // the ray being traversed (object space inside a BLAS)
    D3 wO = O, wD = O, wrD = O;        // TLAS: the world-space ray
    double ht = 0, hu = 0, hv = 0, tIn = 0;
    SphereRayDbl sr{0, 0};             // SPH: the sphere test's factors for this ray (this instance), from the incoming hit.t (tIn)
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
                    if (SPH && !TLAS) sr = sphere_ray_dbl(D.x, D.y, D.z, tIn);
                    found = false; triWon = false; haveNode = true; inBlas = false; node = 0; primLeft = 0; instLeft = 0; st.sp = 0;
                    nodes = q.nodes; recs = q.tris;
                    active = true;
                }
            }
            if (wave_ballot(active) == 0) break;
        }
        if (!active) continue;

        bool done = false;
        if (SPH && primLeft != 0 && sphBlas) {
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
        } else if (SPH && TLAS && primLeft != 0) {
            // ---- one triangle of a triangle BLAS beside sphere BLASes: the test below through tri_test_dbl (the header comment says why) ----
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
        } else if (!SPH && primLeft != 0) {
            // ---- one triangle (tiny_bvh.h:8177-8201, 8302-8316) ----
            const double2* tr = (const double2*)(recs + primPtr);
            const double2 t0 = tr[0], t1 = tr[1], t2 = tr[2], t3 = tr[3], t4 = tr[4];
            primPtr++; primLeft--;
            const D3 v0{t0.x, t0.y, t1.x}, e1{t1.y, t2.x, t2.y}, e2{t3.x, t3.y, t4.x};
            const uint64_t prim = (uint64_t)__double_as_longlong(t4.y);
            const D3 h = cross(D, e2);
            const double a = dot(e1, h);
            if (!(fabs(a) < 0.0000001)) {
                const double f = 1 / a;
                const D3 s = sub(O, v0);
                const double u = f * dot(s, h);
                const D3 qv = cross(s, e1);
                const double v = f * dot(D, qv);
                if (!(u < 0 || v < 0 || u + v > 1)) {
                    const double t = f * dot(e2, qv);
                    const uint64_t inst = TLAS ? curInst : rayInst;
                    if (ANYHIT) {
                        if (t > 0 && t < ht) { found = true; done = true; }
                    } else if (t > 0 && hit_wins_dbl(t, prim, inst, found, ht, hprim, hinst)) {
                        found = true; ht = t; hu = u; hv = v; hprim = prim; hinst = inst;
                    }
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
                nodes = b.nodes; recs = b.tris;
                if (SPH) {   // the tag bit: this BLAS holds spheres
                    const uintptr_t rp = (uintptr_t)b.tris;
                    recs = (const TriDbl*)(rp & ~(uintptr_t)1);
                    sphBlas = (rp & 1) != 0;
                    if (sphBlas) sr = sphere_ray_dbl(D.x, D.y, D.z, tIn);
                }
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
                if (!SPH || (TLAS && triWon)) r[5] = make_double2(hu, hv);
                r[6] = make_double2(__longlong_as_double((long long)hinst), __longlong_as_double((long long)hprim));
            }
            active = false;
        }
    }
    if (st.overflow) atomicOr(status, 1u);
}

// upload helper: {v0, e1 = v1 - v0, e2 = v2 - v0, prim} per primIdx entry, the subtractions BVH_Double::Intersect performs per test (tiny_bvh.h:8178-8179)
__global__ void k_gather_tris_dbl(const uint64_t* __restrict__ primIdx, const double* __restrict__ verts, TriDbl* __restrict__ out, uint64_t nIdx) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nIdx) return;
    const uint64_t p = primIdx[i];   // (< triCount: validated at upload)
    const double* v = verts + p * 9;
    TriDbl r;
    for (int k = 0; k < 3; k++) { r.v0[k] = v[k]; r.e1[k] = v[3 + k] - v[k]; r.e2[k] = v[6 + k] - v[k]; }
    r.prim = p;
    out[i] = r;
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

void launch_double(bool spheres, bool anyhit, bool tlas, const DoubleArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s) {
    using Kernel = void (*)(DoubleArgs, uint32_t*);
    static const Kernel forms[8] = {k_double<false, false, false>, k_double<false, false, true>, k_double<false, true, false>, k_double<false, true, true>,
                                    k_double<true, false, false>,  k_double<true, false, true>,  k_double<true, true, false>,  k_double<true, true, true>};
    hipLaunchKernelGGL(forms[spheres * 4 + anyhit * 2 + tlas], dim3(blocks), dim3(WG), 0, s, q, status);
}

void launch_gather_tris_dbl(const uint64_t* primIdx, const void* verts72, void* recs80, uint64_t nIdx, hipStream_t s) {
    const uint32_t bs = 256;
    hipLaunchKernelGGL(k_gather_tris_dbl, dim3((uint32_t)((nIdx + bs - 1) / bs)), dim3(bs), 0, s, primIdx, (const double*)verts72, (TriDbl*)recs80, nIdx);
}

void launch_gather_spheres_dbl(const uint64_t* primIdx, const void* spheres32, void* recs48, uint64_t nIdx, hipStream_t s) {
    const uint32_t bs = 256;
    hipLaunchKernelGGL(k_gather_spheres_dbl, dim3((uint32_t)((nIdx + bs - 1) / bs)), dim3(bs), 0, s, primIdx, (const SphereDbl*)spheres32, (SphereRecDbl*)recs48, nIdx);
}

}  // namespace tbvh
