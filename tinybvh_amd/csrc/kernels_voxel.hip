// kernels_voxel.hip — VoxelSet Intersect / IsOccluded (and both under a TLAS) for gfx950 (MI355X).
//
// One DDA, four instantiations (closest / any hit x one voxel set / a BVH_GPU-format TLAS over BLASInstance records), restating
// VoxelSet::Setup3DDDA / Intersect / IsOccluded (tiny_bvh.h:3829-4156) operation for operation — tests/oracle_voxel.c is the same walk in
// C, pinned bit for bit against the real reference:
//   - three levels over the unit cube: 8^3 top cells (one occupancy bit each), 4^3 grid cells per top cell (a brick index each, 0 = empty),
//     8^3 voxels per brick (the value; 0 = empty); the first filled voxel is the set's candidate, at t = the entry distance of its cell;
//   - a ray outside the cube enters it by the slab test with the ternary min / max (tiny_bvh.h:445-446) and is dropped if it misses, enters
//     beyond hit.t, or lies behind (3832-3843);
//   - per level the point along the ray is fmaf(D, t + 0.0000025f, O) * dim: the reference build (g++ -O3 -mavx2 -mfma) contracts
//     O + D * (t + eps) into one fused multiply-add per component (3846 / 3895 / 3911 / 4045 / 4061); the plane expressions are fused
//     there too, but their products are exact powers of two.  This file is built with -ffp-contract=off: nothing else is fused;
//   - the sign of D from its float bits (-0.0 steps negative), planes ceilf(p) - sign, cells (int)p with x86 semantics (cvttss2si gives
//     INT_MIN for NaN and out-of-range values; v_cvt_i32_f32 would saturate and give 0 for NaN), tinybvh_clamp's int32 overload (458) —
//     also for the unsigned brick offsets of 3912-3914 / 4062-4064, so a negative offset clamps to 0 —, strict < between the axes;
//   - TLAS instances as in kernels_tlas.hip: mask test, invTransform with the w divide and the reference build's contraction
//     (oracle/tbvh_oracle.c: orc_xform_point / orc_xform_vec), D not renormalised, rD = tinybvh_safercp(D'); node culls with cull_bound.
// Acceptance (DESIGN.md par. 10): a candidate is recorded only if it wins against the record's current hit by the library's rule — t < hit.t,
// or at equal t a found hit with a larger prim, then a larger instance.  The walk is not cut short by the t it has reached: t can step BACK
// (a zero direction component with the origin on a cell plane gives a finer level's plane distance 0 x 1e30 = 0).  The reference writes the first filled voxel unconditionally (3920-3935), so a finite tmax or a nearer TLAS hit can get a
// FARTHER one there; with tmax = 1e30 and no TLAS the records are the reference's.  Occlusion is the reference's: the first filled voxel,
// t < hit.t, and the walk ends when the top-level t is no longer below hit.t (4040).
//
// ONE flat loop per lane: an iteration visits one cell of the lane's current level (one load) and, unless it descends, takes one DDA step.
// Lanes at different levels run the same code; the level's constants are selects, its DDA state lives in one set of registers (the
// parent levels' is saved on descent, restored on ascent).  Persistent one-wave workgroups with per-lane ray replacement (ray_pool.h).
// A voxel set is ONE array of uint32: [top grid 16 | grid 32768 | bricks n_bricks x 512] (capi_voxel.hip), every index in it validated
// at upload, so every load below is in bounds.
#include "device_common.h"
#include "lane_stack.h"
#include "ray_pool.h"
#include "kernels.h"
#include "voxel_edit.h"

namespace tbvh {

namespace {

constexpr int WG = 64;
constexpr int LDS_N = 16;
constexpr int REFILL_MIN = 16;
constexpr uint32_t kGridOff = 16u, kBrickOff = 16u + 32768u;

__device__ __forceinline__ float vmin(float a, float b) { return a < b ? a : b; }   // tinybvh_min (tiny_bvh.h:445)
__device__ __forceinline__ float vmax(float a, float b) { return a > b ? a : b; }   // tinybvh_max (tiny_bvh.h:446)
__device__ __forceinline__ int32_t vclamp(int32_t x, int32_t a, int32_t b) { return x > a ? (x < b ? x : b) : a; }   // tiny_bvh.h:458
__device__ __forceinline__ int32_t cvt_x86(float f) { return voxel_cvt_x86(f); }   // (voxel_edit.h: shared with the voxelise step)
__device__ __forceinline__ float safercp(float x) {   // tinybvh_safercp (tiny_bvh.h:442)
    if (x > 1e-12f || x < -1e-12f) return 1.0f / x;
    return x >= 0 ? kFar : -kFar;
}
__device__ __forceinline__ float fmin3(float a, float b, float c) { return __builtin_fminf(__builtin_fminf(a, b), c); }
__device__ __forceinline__ float fmax3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }

// The DDA state of one lane in one voxel set.  Level 0 = top cells, 1 = grid cells, 2 = voxels; the current level's cell, plane distances
// and steps are X / tm / td, the parents' are kept in X1 / tm1 (level 0) and X2 / tm2 (level 1) while a child level runs.
struct Dda {
    const uint32_t* vox;
    float3 O, D, rD;
    float t;
    uint32_t lvl;
    bool pend;           // the current cell has been visited: step next
    uint32_t X, Y, Z;
    float3 tm, td;
    uint32_t X1, Y1, Z1, X2, Y2, Z2;
    float3 tm1, tm2, td1;
};

__device__ __forceinline__ uint32_t sbit(float d) { return __float_as_uint(d) >> 31; }

// a level's cell and plane distances at the current t (Setup3DDDA 3845-3852; 3895-3902; 3911-3917): dim = 8 / 32 / 256;
// cell = clamp((int)p - sub, lo, lo + span) - lo in 32-bit wrapping arithmetic
__device__ __forceinline__ void dda_enter(Dda& s, float dim, float rdim, uint32_t subX, uint32_t subY, uint32_t subZ, uint32_t loX, uint32_t loY, uint32_t loZ,
                                          int32_t span) {
    const float e = s.t + 0.0000025f;
    const float px = __builtin_fmaf(s.D.x, e, s.O.x) * dim, py = __builtin_fmaf(s.D.y, e, s.O.y) * dim, pz = __builtin_fmaf(s.D.z, e, s.O.z) * dim;
    s.X = (uint32_t)vclamp((int32_t)((uint32_t)cvt_x86(px) - subX), (int32_t)loX, (int32_t)loX + span) - loX;
    s.Y = (uint32_t)vclamp((int32_t)((uint32_t)cvt_x86(py) - subY), (int32_t)loY, (int32_t)loY + span) - loY;
    s.Z = (uint32_t)vclamp((int32_t)((uint32_t)cvt_x86(pz) - subZ), (int32_t)loZ, (int32_t)loZ + span) - loZ;
    const float gx = (__builtin_ceilf(px) - (float)sbit(s.D.x)) * rdim, gy = (__builtin_ceilf(py) - (float)sbit(s.D.y)) * rdim,
                gz = (__builtin_ceilf(pz) - (float)sbit(s.D.z)) * rdim;
    s.tm = make_float3((gx - s.O.x) * s.rD.x, (gy - s.O.y) * s.rD.y, (gz - s.O.z) * s.rD.z);
}

// Setup3DDDA (3829-3853): false when the ray misses the cube, enters it beyond hitT or lies behind it
__device__ __forceinline__ bool dda_setup(Dda& s, float hitT) {
    s.t = 0;
    if (!(s.O.x >= 0 && s.O.x <= 1 && s.O.y >= 0 && s.O.y <= 1 && s.O.z >= 0 && s.O.z <= 1)) {
        const float tx1 = -s.O.x * s.rD.x, tx2 = (1 - s.O.x) * s.rD.x;
        float tmin = vmin(tx1, tx2), tmax = vmax(tx1, tx2);
        const float ty1 = -s.O.y * s.rD.y, ty2 = (1 - s.O.y) * s.rD.y;
        tmin = vmax(tmin, vmin(ty1, ty2));
        tmax = vmin(tmax, vmax(ty1, ty2));
        const float tz1 = -s.O.z * s.rD.z, tz2 = (1 - s.O.z) * s.rD.z;
        tmin = vmax(tmin, vmin(tz1, tz2));
        tmax = vmin(tmax, vmax(tz1, tz2));
        if (tmax < tmin || tmin > hitT || tmax < 0) return false;
        s.t = tmin;
    }
    dda_enter(s, 8.0f, 1.0f / 8.0f, 0u, 0u, 0u, 0u, 0u, 0u, 7);
    const float sx = 1.0f - 2.0f * (float)sbit(s.D.x), sy = 1.0f - 2.0f * (float)sbit(s.D.y), sz = 1.0f - 2.0f * (float)sbit(s.D.z);
    s.td = make_float3((sx * (1.0f / 8.0f)) * s.rD.x, (sy * (1.0f / 8.0f)) * s.rD.y, (sz * (1.0f / 8.0f)) * s.rD.z);
    s.td1 = s.td;
    s.lvl = 0; s.pend = false;
    return true;
}

enum : uint32_t { DDA_RUN = 0, DDA_HIT = 1, DDA_OUT = 2 };

// One iteration: visit the current cell (one load) or take the pending step.  Occlusion ends the walk at the head of a top-level visit once
// t is no longer below hitT (`while (t < hit.t)`, 4040).  DDA_HIT leaves the voxel value in val.
template <bool ANYHIT>
__device__ __forceinline__ uint32_t dda_iter(Dda& s, float hitT, uint32_t& val) {
    if (!s.pend) {
        uint32_t off, bit = 0;
        if (s.lvl == 0) {
            if (ANYHIT && !(s.t < hitT)) return DDA_OUT;
            const uint32_t ti = s.X + s.Y * 8u + s.Z * 64u;
            off = ti >> 5; bit = ti & 31u;
        } else if (s.lvl == 1) off = kGridOff + s.X1 * 4u + s.Y1 * 128u + s.Z1 * 4096u + s.X + s.Y * 32u + s.Z * 1024u;   // gridBase (3901) + cell
        else off = val + s.X + s.Y * 8u + s.Z * 64u;   // (val: the brick's base while in it)
        const uint32_t w = s.vox[off];
        const bool filled = s.lvl == 0 ? ((w >> bit) & 1u) != 0 : w != 0;
        if (filled) {
            if (s.lvl == 2) { val = w; return DDA_HIT; }
            if (s.lvl == 0) {   // into the top cell's 4^3 grid cells (3893-3902)
                s.X1 = s.X; s.Y1 = s.Y; s.Z1 = s.Z; s.tm1 = s.tm;
                dda_enter(s, 32.0f, 1.0f / 32.0f, 0u, 0u, 0u, s.X1 * 4u, s.Y1 * 4u, s.Z1 * 4u, 3);
                s.td = make_float3(s.td1.x * 0.25f, s.td1.y * 0.25f, s.td1.z * 0.25f);
                s.lvl = 1;
            } else {            // into the brick (3908-3917)
                s.X2 = s.X; s.Y2 = s.Y; s.Z2 = s.Z; s.tm2 = s.tm;
                dda_enter(s, 256.0f, 1.0f / 256.0f, (s.X2 + s.X1 * 4u) * 8u, (s.Y2 + s.Y1 * 4u) * 8u, (s.Z2 + s.Z1 * 4u) * 8u, 0u, 0u, 0u, 7);
                const float3 td2 = make_float3(s.td1.x * 0.25f, s.td1.y * 0.25f, s.td1.z * 0.25f);
                s.td = make_float3(td2.x * 0.125f, td2.y * 0.125f, td2.z * 0.125f);
                val = kBrickOff + w * 512u;
                s.lvl = 2;
            }
            return DDA_RUN;
        }
    }
    // one step at this level (3937-3965 and its two copies); leaving the level resumes the parent with ITS pending step
    s.pend = false;
    const uint32_t lim = s.lvl == 1 ? 4u : 8u;
    const int32_t stx = 1 - 2 * (int32_t)sbit(s.D.x), sty = 1 - 2 * (int32_t)sbit(s.D.y), stz = 1 - 2 * (int32_t)sbit(s.D.z);
    bool out;
    if (s.tm.x < s.tm.y) {
        if (s.tm.x < s.tm.z) { s.X += (uint32_t)stx; out = s.X >= lim; if (!out) { s.t = s.tm.x; s.tm.x += s.td.x; } }
        else { s.Z += (uint32_t)stz; out = s.Z >= lim; if (!out) { s.t = s.tm.z; s.tm.z += s.td.z; } }
    } else {
        if (s.tm.y < s.tm.z) { s.Y += (uint32_t)sty; out = s.Y >= lim; if (!out) { s.t = s.tm.y; s.tm.y += s.td.y; } }
        else { s.Z += (uint32_t)stz; out = s.Z >= lim; if (!out) { s.t = s.tm.z; s.tm.z += s.td.z; } }
    }
    if (out) {
        if (s.lvl == 0) return DDA_OUT;
        if (s.lvl == 2) {
            s.X = s.X2; s.Y = s.Y2; s.Z = s.Z2; s.tm = s.tm2;
            s.td = make_float3(s.td1.x * 0.25f, s.td1.y * 0.25f, s.td1.z * 0.25f);
            s.lvl = 1;
        } else {
            s.X = s.X1; s.Y = s.Y1; s.Z = s.Z1; s.tm = s.tm1; s.td = s.td1;
            s.lvl = 0;
        }
        s.pend = true;
    }
    return DDA_RUN;
}

// the library's rule for a voxel candidate (device_common.h: hit_wins, with the strict comparison against the incoming tmax)
__device__ __forceinline__ bool vox_wins(float t, uint32_t prim, uint32_t inst, bool found, float bestT, uint32_t bestPrim, uint32_t bestInst) {
    return t < bestT || (found && t == bestT && (prim < bestPrim || (prim == bestPrim && inst < bestInst)));
}

template <bool ANYHIT, bool TLAS>
__global__ __launch_bounds__(WG) void k_voxel(const uint32_t* __restrict__ vox, const float4* __restrict__ tlasNodes, const uint32_t* __restrict__ tlasIdx,
                                              const float4* __restrict__ instances, const BlasDesc* __restrict__ blas, QueryArgs q, uint32_t* __restrict__ status) {
    enum : uint32_t { M_TLAS = 0, M_INST = 1, M_VOX = 2 };
    __shared__ uint32_t stk[TLAS ? LDS_N : 1][WG];
    LaneStack<uint32_t, TLAS ? LDS_N : 1, WG> st;
    st.init(&stk[0][threadIdx.x], q.spill + (blockIdx.x * WG + threadIdx.x), (size_t)gridDim.x * WG, q.spillStride);
    RayPool<64> pool;
    const uint64_t nRaysTotal = q.nRaysDev ? *q.nRaysDev : q.nRays;
    pool.init(q.poolParts, q.counterNext);

    bool active = false, found = false;
    uint64_t ri = 0;
    Dda s;
    s.vox = vox;
    float3 wO = make_float3(0, 0, 0), wD = wO, wrD = wO;   // the ray as the caller gave it
    float4 hit = make_float4(0, 0, 0, 0);                  // t, u, v, prim
    uint32_t hitInst = 0, rayMask = 0, rayInst = 0, mode = M_VOX, node = 0, leafNext = 0, leafEnd = 0, curInst = 0, bval = 0;

    for (;;) {
        const uint32_t nIdle = wave_count(!active);
        if (nIdle >= (uint32_t)REFILL_MIN) {
            if (!pool.dry()) {
                uint64_t nri = 0;
                if (pool.acquire(!active, q.counter, nRaysTotal, nri)) {
                    ri = nri;
                    const RayRec* rp = q.rays + ri;
                    wO = xyz(rp->O); wD = xyz(rp->D); wrD = xyz(rp->rD);
                    rayMask = as_u32(rp->O.w); rayInst = as_u32(rp->D.w);
                    hit = q.fresh ? make_float4(q.freshTmax, 0.f, 0.f, 0.f) : rp->hit;
                    hitInst = as_u32(rp->rD.w);
                    found = false; st.sp = 0; node = 0;
                    active = true;
                    if (TLAS) mode = M_TLAS;
                    else {
                        s.O = wO; s.D = wD; s.rD = wrD;
                        if (dda_setup(s, hit.x)) mode = M_VOX;
                        else mode = M_INST;   // (BLAS: nothing more to do)
                    }
                }
            }
            if (wave_ballot(active) == 0) break;
        }
        if (!active) continue;
        bool done = false;

        if (mode == M_VOX) {
            uint32_t v = bval;
            const uint32_t r = dda_iter<ANYHIT>(s, hit.x, v);
            bval = v;
            bool leave = r == DDA_OUT;
            if (r == DDA_HIT) {
                leave = true;
                const uint32_t inst = TLAS ? curInst : rayInst;
                if (ANYHIT) { if (s.t < hit.x) { found = true; done = true; } }   // 4038
                else if (vox_wins(s.t, v, inst, found, hit.x, as_u32(hit.w), hitInst)) {
                    found = true; hit.x = s.t; hit.w = as_f32(v); hitInst = inst;
                }
            }
            if (leave && !done) {
                if (TLAS) mode = M_INST;
                else done = true;
            }
        } else if (!TLAS) {
            done = true;   // (missed the cube at setup)
        } else if (mode == M_INST) {
            if (leafNext == leafEnd) {   // TLAS leaf done
                if (st.sp == 0) done = true;
                else { node = st.pop(); mode = M_TLAS; }
            } else {
                const uint32_t ii = tlasIdx[leafNext++];
                const float4* ip = instances + (size_t)ii * 12;
                const float4 b0 = ip[8], b1 = ip[9];                      // aabbMin|blasIdx, aabbMax|mask
                if (as_u32(b1.w) & rayMask) {                              // tiny_bvh.h:3326
                    const float4 r0 = ip[4], r1 = ip[5], r2 = ip[6], r3 = ip[7];   // invTransform rows
                    // tinybvh_transform_point / _vector with the reference build's contraction (voxel_edit.h, shared with the normals of a TLAS hit)
                    float3 lO, lD;
                    voxel_instance_ray(r0, r1, r2, r3, wO, wD, lO, lD);
                    s.O = lO;
                    s.D = lD;
                    s.rD = make_float3(safercp(lD.x), safercp(lD.y), safercp(lD.z));
                    s.vox = (const uint32_t*)blas[as_u32(b0.w)].nodes;
                    curInst = ii;
                    if (dda_setup(s, hit.x)) mode = M_VOX;
                }
            }
        } else {
            // one TLAS node (SLAB_TEST_TWO_NODES form, as kernels_tlas.hip)
            const float4 n0 = tlasNodes[node * 4], n1 = tlasNodes[node * 4 + 1], n2 = tlasNodes[node * 4 + 2], n3 = tlasNodes[node * 4 + 3];
            const uint32_t cnt = as_u32(n2.w);
            if (cnt) { leafNext = as_u32(n3.w); leafEnd = leafNext + cnt; mode = M_INST; }
            else {
                const float3 rD = wrD, O = wO;
                const float3 ro = make_float3(O.x * rD.x, O.y * rD.y, O.z * rD.z);
                const float lx1 = __builtin_fmaf(n0.x, rD.x, -ro.x), lx2 = __builtin_fmaf(n1.x, rD.x, -ro.x);
                const float ly1 = __builtin_fmaf(n0.y, rD.y, -ro.y), ly2 = __builtin_fmaf(n1.y, rD.y, -ro.y);
                const float lz1 = __builtin_fmaf(n0.z, rD.z, -ro.z), lz2 = __builtin_fmaf(n1.z, rD.z, -ro.z);
                const float rx1 = __builtin_fmaf(n2.x, rD.x, -ro.x), rx2 = __builtin_fmaf(n3.x, rD.x, -ro.x);
                const float ry1 = __builtin_fmaf(n2.y, rD.y, -ro.y), ry2 = __builtin_fmaf(n3.y, rD.y, -ro.y);
                const float rz1 = __builtin_fmaf(n2.z, rD.z, -ro.z), rz2 = __builtin_fmaf(n3.z, rD.z, -ro.z);
                const float tminL = __builtin_fmaxf(fmax3(__builtin_fminf(lx1, lx2), __builtin_fminf(ly1, ly2), __builtin_fminf(lz1, lz2)), 0.0f);
                const float tmaxL = __builtin_fminf(fmin3(__builtin_fmaxf(lx1, lx2), __builtin_fmaxf(ly1, ly2), __builtin_fmaxf(lz1, lz2)), cull_bound(hit.x));
                const float tminR = __builtin_fmaxf(fmax3(__builtin_fminf(rx1, rx2), __builtin_fminf(ry1, ry2), __builtin_fminf(rz1, rz2)), 0.0f);
                const float tmaxR = __builtin_fminf(fmin3(__builtin_fmaxf(rx1, rx2), __builtin_fmaxf(ry1, ry2), __builtin_fmaxf(rz1, rz2)), cull_bound(hit.x));
                const bool hL = tmaxL >= tminL, hR = tmaxR >= tminR;
                uint32_t l = as_u32(n0.w), r = as_u32(n1.w);
                if (hL && hR) {
                    if (tminL > tminR) { const uint32_t t = l; l = r; r = t; }
                    st.push(r);
                    node = l;
                } else if (hL) node = l;
                else if (hR) node = r;
                else {
                    if (st.sp == 0) done = true;
                    else node = st.pop();
                }
            }
        }
        if (done) {
            RayRec* rp = q.rays + ri;
            if (ANYHIT) q.occluded[ri] = found ? 1 : 0;
            else if (found) { rp->hit = hit; ((uint32_t*)rp)[11] = hitInst; }   // byte 44 = hit.inst; u, v as they were (fresh: 0)
            else if (q.fresh) rp->hit = hit;
            active = false;
        }
    }
    if (TLAS && st.overflow) atomicOr(status, 1u);
}

}  // namespace

void launch_voxel(bool anyhit, const uint32_t* vox, const float4* tlasNodes, const uint32_t* tlasIdx, const float4* instances, const BlasDesc* blas,
                  const QueryArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s) {
    if (tlasNodes) {
        if (anyhit) hipLaunchKernelGGL((k_voxel<true, true>), dim3(blocks), dim3(WG), 0, s, vox, tlasNodes, tlasIdx, instances, blas, q, status);
        else hipLaunchKernelGGL((k_voxel<false, true>), dim3(blocks), dim3(WG), 0, s, vox, tlasNodes, tlasIdx, instances, blas, q, status);
    } else {
        if (anyhit) hipLaunchKernelGGL((k_voxel<true, false>), dim3(blocks), dim3(WG), 0, s, vox, tlasNodes, tlasIdx, instances, blas, q, status);
        else hipLaunchKernelGGL((k_voxel<false, false>), dim3(blocks), dim3(WG), 0, s, vox, tlasNodes, tlasIdx, instances, blas, q, status);
    }
}

}  // namespace tbvh
