// voxel_edit.h — the rules and the arithmetic of editing a VoxelSet (tiny_bvh.h:3786-3827) and of VoxelSet::GetNormal (3860-3869), one copy for
// the kernels (kernels_voxel_edit.hip, kernels_voxel.hip), the device entry points (capi_voxel_edit.hip) and the CPU twins (voxel_edit_host.cpp,
// capi_voxel.hip).  Everything that includes this is built -ffp-contract=off: the fused multiply-adds below are the ones the reference's object
// code has (g++ -O3 -mavx2 -mfma; DESIGN.md par. 21), and the only ones.
//
//   Set( x, y, z, v ): grid cell g = x / 8 + 32 ( y / 8 ) + 1024 ( z / 8 ); a cell without a brick takes the next free one (freeBrickPtr, brick 0
//                      skipped) — also when v == 0 —; the voxel ( x & 7 ) + 8 ( y & 7 ) + 64 ( z & 7 ) of that brick becomes v.  HERE a coordinate
//                      beyond 255 is refused; the reference has no check and would write outside its grid.
//   UpdateTopGrid:     bit x + 8 y + 64 z of the 512 is set when any of the 4^3 grid cells of that group holds a brick.
//   GetNormal:         I = fma( t, D, O ) * 256 per component (ONE fused multiply-add: vfmadd213ss in the reference build, then vmulss),
//                      f = I - floorf( I ), d = f < 1 - f ? f : 1 - f, m = min( min( d.x, d.y ), d.z ) with the same ternary; the first of x, y, z
//                      with m == d answers (a NaN answers z), with D > 0 ? -1 : 1 on that axis: a zero or negative-zero component gives +1.
//   instance space:    tinybvh_transform_point / _vector by the instance's invTransform with the w divide and the reference build's contraction
//                      (oracle/tbvh_oracle.c: orc_xform_point / orc_xform_vec), D not renormalised — what k_voxel does on entering an instance.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TBVH_VOXEL_HD __host__ __device__ __forceinline__
#else
#define TBVH_VOXEL_HD inline
#endif

namespace tbvh {

#if !defined(__HIPCC__)
// a plain C++ compile (voxel_edit_host.cpp, also on its own under a sanitizer) has no HIP vector types: the few this header names
struct float3 { float x, y, z; };
struct alignas(16) float4 { float x, y, z, w; };
inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
#endif

constexpr uint32_t kVoxObjDim = 256, kVoxBrickDim = 8, kVoxGridDim = 32, kVoxGroupDim = 4, kVoxTopDim = 8;   // VoxelSet::objectDim = 256 (tiny_bvh.h:1008-1022)
constexpr uint32_t kVoxGridWords = kVoxGridDim * kVoxGridDim * kVoxGridDim, kVoxBrickWords = kVoxBrickDim * kVoxBrickDim * kVoxBrickDim, kVoxTopWords = 16;
constexpr uint64_t kVoxMaxBricks = 1ull << 22;   // (device offsets are 32-bit: 16 + 32768 + 2^22 x 512 < 2^31)
constexpr uint32_t kVoxGridOff = kVoxTopWords, kVoxBrickOff = kVoxTopWords + kVoxGridWords;   // the one allocation: [top 16 | grid 32768 | bricks cap x 512]
constexpr uint32_t kStatusVoxelNormal = 1024u;   // status word: a hit record's instance index is not an instance of the TLAS (capi_query.hip: checkStatus)

TBVH_VOXEL_HD bool voxel_in_range(uint32_t x, uint32_t y, uint32_t z) { return (x | y | z) < kVoxObjDim; }
TBVH_VOXEL_HD uint32_t voxel_grid_cell(uint32_t x, uint32_t y, uint32_t z) {
    return x / kVoxBrickDim + (y / kVoxBrickDim) * kVoxGridDim + (z / kVoxBrickDim) * kVoxGridDim * kVoxGridDim;
}
TBVH_VOXEL_HD uint32_t voxel_in_brick(uint32_t x, uint32_t y, uint32_t z) {
    return (x & (kVoxBrickDim - 1)) + (y & (kVoxBrickDim - 1)) * kVoxBrickDim + (z & (kVoxBrickDim - 1)) * kVoxBrickDim * kVoxBrickDim;
}
// the first grid cell of top cell ti = x + 8 y + 64 z, and whether any of its 4^3 cells holds a brick (UpdateTopGrid's inner loops)
TBVH_VOXEL_HD bool voxel_group_filled(const uint32_t* grid, uint32_t ti) {
    const uint32_t x = ti & 7u, y = (ti >> 3) & 7u, z = ti >> 6;
    const uint32_t* base = grid + x * kVoxGroupDim + y * kVoxGroupDim * kVoxGridDim + z * kVoxGroupDim * kVoxGridDim * kVoxGridDim;
    bool has = false;
    for (uint32_t w = 0; w < kVoxGroupDim; w++) for (uint32_t v = 0; v < kVoxGroupDim; v++) for (uint32_t u = 0; u < kVoxGroupDim; u++)
        has |= base[u + v * kVoxGridDim + w * kVoxGridDim * kVoxGridDim] != 0;
    return has;
}

// (int)f as x86 performs it (cvttss2si gives INT_MIN for NaN and out-of-range values; v_cvt_i32_f32 would saturate and give 0 for NaN), and
// tinybvh_clamp's int32 overload (tiny_bvh.h:458): shared by the DDA (kernels_voxel.hip) and the voxelise step
TBVH_VOXEL_HD int32_t voxel_cvt_x86(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int32_t)f : INT32_MIN; }
TBVH_VOXEL_HD int32_t voxel_clamp(int32_t x, int32_t a, int32_t b) { return x > a ? (x < b ? x : b) : a; }

// ---- voxelising a traced scene (tiny_bvh_foliage.cpp:222-258; DESIGN.md par. 21): 3 x 256^2 axis rays, ray id = a * 65536 + x * 256 + y -------------
// The reference build's object code (tests/voxel_edit_ref_shim.cpp, g++ -O3 -mavx2 -mfma): fx = (float)x * (1 / 256) (vmulss), then
// O[u] = fma( fx, maxSize, bmin[u] ) — ONE fused multiply-add (vfmadd132ss) —, O[a] = bmin[a] - 0.0001f (vsubss); I = fma( D, t, O ) and
// O' = fma( D, 0.0001f, I ), exact products both (D is a unit axis); P[a] = (int)( ( 256 * ( I[a] - bmin[a] ) ) * reciExt ): vsubss, vmulss, vmulss, vcvttss2si.
constexpr uint32_t kVoxelizeRays = 3u * 65536u;
struct VoxelizeArgs { float bmin[3]; float maxSize; float reciExt[3]; uint32_t color; uint32_t maxHits; };
// origin of ray id (direction: the unit vector of axis a = id >> 16)
TBVH_VOXEL_HD void voxelize_origin(const VoxelizeArgs& p, uint32_t id, float O[3]) {
    const uint32_t a = id >> 16, u = (a + 1u) % 3u, v = (a + 2u) % 3u;
    const float fx = (float)((id >> 8) & 255u) * (1.0f / 256.0f), fy = (float)(id & 255u) * (1.0f / 256.0f);
    O[a] = p.bmin[a] - 0.0001f;
    O[u] = __builtin_fmaf(fx, p.maxSize, p.bmin[u]);
    O[v] = __builtin_fmaf(fy, p.maxSize, p.bmin[v]);
}
// the voxel a hit at I[a] (on axis a of ray id) lands in: P[u] = x, P[v] = y, P[a] from the hit point, each clamped to 0..255
TBVH_VOXEL_HD void voxelize_cell(const VoxelizeArgs& p, uint32_t id, float Ia, uint32_t P[3]) {
    const uint32_t a = id >> 16, u = (a + 1u) % 3u, v = (a + 2u) % 3u;
    P[u] = (id >> 8) & 255u; P[v] = id & 255u;
    P[a] = (uint32_t)voxel_clamp(voxel_cvt_x86(((float)kVoxObjDim * (Ia - p.bmin[a])) * p.reciExt[a]), 0, (int32_t)kVoxObjDim - 1);
}
// ( (int)( r * 255 ) << 16 ) + ( (int)( g * 255 ) << 8 ) + (int)( b * 255 ) (tiny_bvh_foliage.cpp:251-252), in wrapping 32-bit arithmetic
TBVH_VOXEL_HD uint32_t voxelize_value(float r, float g, float b) {
    return ((uint32_t)voxel_cvt_x86(r * 255.0f) << 16) + ((uint32_t)voxel_cvt_x86(g * 255.0f) << 8) + (uint32_t)voxel_cvt_x86(b * 255.0f);
}

TBVH_VOXEL_HD float voxel_tmin(float a, float b) { return a < b ? a : b; }   // tinybvh_min (tiny_bvh.h:445)

// VoxelSet::GetNormal (3860-3869) from O, D and hit.t
TBVH_VOXEL_HD float4 voxel_normal(float3 O, float3 D, float t) {
    const float ix = __builtin_fmaf(t, D.x, O.x) * (float)kVoxObjDim, iy = __builtin_fmaf(t, D.y, O.y) * (float)kVoxObjDim, iz = __builtin_fmaf(t, D.z, O.z) * (float)kVoxObjDim;
    const float fx = ix - __builtin_floorf(ix), fy = iy - __builtin_floorf(iy), fz = iz - __builtin_floorf(iz);
    const float dx = voxel_tmin(fx, 1.0f - fx), dy = voxel_tmin(fy, 1.0f - fy), dz = voxel_tmin(fz, 1.0f - fz);
    const float m = voxel_tmin(voxel_tmin(dx, dy), dz);
    if (m == dx) return make_float4(D.x > 0 ? -1.0f : 1.0f, 0.f, 0.f, 0.f);
    if (m == dy) return make_float4(0.f, D.y > 0 ? -1.0f : 1.0f, 0.f, 0.f);
    return make_float4(0.f, 0.f, D.z > 0 ? -1.0f : 1.0f, 0.f);
}

// a ray into an instance's space: r0..r3 = the rows of BLASInstance::invTransform (float4 4..7 of the 192-byte record)
TBVH_VOXEL_HD void voxel_instance_ray(float4 r0, float4 r1, float4 r2, float4 r3, float3 O, float3 D, float3& lO, float3& lD) {
    const float px = __builtin_fmaf(r0.z, O.z, __builtin_fmaf(r0.x, O.x, r0.y * O.y)) + r0.w;
    const float py = __builtin_fmaf(r1.z, O.z, __builtin_fmaf(r1.x, O.x, r1.y * O.y)) + r1.w;
    const float pz = __builtin_fmaf(r2.z, O.z, __builtin_fmaf(r2.x, O.x, r2.y * O.y)) + r2.w;
    const float w = __builtin_fmaf(r3.z, O.z, __builtin_fmaf(r3.x, O.x, r3.y * O.y)) + r3.w;
    lD = make_float3(__builtin_fmaf(r0.z, D.z, __builtin_fmaf(r0.x, D.x, r0.y * D.y)), __builtin_fmaf(r1.z, D.z, __builtin_fmaf(r1.x, D.x, r1.y * D.y)),
                     __builtin_fmaf(r2.z, D.z, __builtin_fmaf(r2.x, D.x, r2.y * D.y)));
    if (w == 1) lO = make_float3(px, py, pz);
    else { const float iw = 1.f / w; lO = make_float3(px * iw, py * iw, pz * iw); }
}

// one record of a normals batch: the ray's O, D, hit.t and hit.inst are floats 0-2, 4-6, 12 and dword 11 of its 64-byte prefix.  A miss
// (hit.t >= 1e30) gets zeros; under a TLAS (instances != nullptr) the ray goes into the hit instance's space first.  false: hit.inst is no instance
// (nothing was read through it; zeros).
TBVH_VOXEL_HD bool voxel_normal_record(const float4* rec, const float4* instances, uint64_t nInst, float4* out) {
    const float4 o = rec[0], d = rec[1], h = rec[3];
    *out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!(h.x < 1e30f)) return true;
    float3 O = make_float3(o.x, o.y, o.z), D = make_float3(d.x, d.y, d.z);
    if (instances) {
        uint32_t inst;
        __builtin_memcpy(&inst, &rec[2].w, 4);
        if (inst >= nInst) return false;
        const float4* ip = instances + (size_t)inst * 12;
        float3 lO, lD;
        voxel_instance_ray(ip[4], ip[5], ip[6], ip[7], O, D, lO, lD);
        O = lO; D = lD;
    }
    *out = voxel_normal(O, D, h.x);
    return true;
}

// ---- the host side of Set / UpdateTopGrid: the arrays as std::vector-like storage the caller grows ----------------------------------------
// VoxelSet::Set on (grid, bricks): `bricks` is a container of uint32 with size() / resize( n, 0 ) holding the USED bricks (brick 0 included); the
// pool's reallocation in the reference does not change the numbering, so a growing vector stands for it
template <class Grid, class Bricks>
inline void voxel_set_host(Grid& grid, Bricks& bricks, uint32_t x, uint32_t y, uint32_t z, uint32_t v) {
    const uint32_t g = voxel_grid_cell(x, y, z);
    uint32_t b = grid[g];
    if (!b) {
        b = grid[g] = (uint32_t)(bricks.size() / kVoxBrickWords);
        bricks.resize(bricks.size() + kVoxBrickWords, 0u);
    }
    bricks[(size_t)b * kVoxBrickWords + voxel_in_brick(x, y, z)] = v;
}
inline void voxel_update_top_grid_host(const uint32_t* grid, uint32_t* top16) {
    for (uint32_t k = 0; k < kVoxTopWords; k++) top16[k] = 0;
    for (uint32_t ti = 0; ti < kVoxTopDim * kVoxTopDim * kVoxTopDim; ti++)
        if (voxel_group_filled(grid, ti)) top16[ti >> 5] |= 1u << (ti & 31);
}


// (voxel_edit_host.cpp) n records { x, y, z, v } set in turn on a host set, refusals first: what tbvh_host_voxelset_set is over a tbvh_hostbvh's arrays
int voxel_host_set_records(std::vector<uint32_t>& grid, std::vector<uint32_t>& bricks, const uint32_t* xyzv, uint64_t n);

}  // namespace tbvh
