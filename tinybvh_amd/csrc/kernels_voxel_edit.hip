// kernels_voxel_edit.hip — editing a VoxelSet on the device for gfx950 (MI355X): the batched VoxelSet::Set, UpdateTopGrid and GetNormal
// (tiny_bvh.h:3786-3827, 3860-3869), and the ray generator and step kernel of the scene-to-voxels loop (tiny_bvh_foliage.cpp:222-258); the rules and the
// arithmetic are voxel_edit.h, DESIGN.md par. 21.
//
// A batch of n records { x, y, z, v } has to leave the arrays as n sequential Set calls would: the last record of a voxel wins, and the grid cells
// that get a brick are numbered in the order of their FIRST record.  Both orders are recovered from record indices with atomicMin / atomicMax, whose
// results do not depend on the order the lanes arrive in, and every store of the last pass has one writer: nothing depends on scheduling.
//   k_voxel_prep    the work area: cellFirst = ~0, cellIds = 0, 1, 2, ..., counters = 0
//   k_voxel_mark    atomicMin( cellFirst[g], i ) for every record i whose grid cell g has no brick; the lane that finds ~0 there counts the cell
//   (sort)          hipcub radix sort of the 32768 ( cellFirst, cell ) pairs: the marked cells come first, in the order of their first record
//   k_voxel_number  grid[ sortedCells[r] ] = used + r for r < nNew
//   k_voxel_winner  atomicMax( winner[ brick * 512 + voxel ], i + 1 )
//   k_voxel_store   record i with winner == i + 1 stores v and writes the winner word back to 0
// Every index is checked before it is an address: a record with a coordinate beyond 255 is skipped by every pass (and counted by the first), grid
// entries are below the used count by the upload's validation and this file's numbering, and the caller (capi_voxel_edit.hip) grows the pool and
// the winner words to hold used + nNew bricks before k_voxel_number runs.
#include <hipcub/hipcub.hpp>

#include "device_common.h"
#include "kernels.h"
#include "voxel_edit.h"

namespace tbvh {

namespace {

constexpr int WG = 256;
constexpr uint32_t kNone = 0xFFFFFFFFu;

__global__ __launch_bounds__(WG) void k_voxel_prep(uint32_t* __restrict__ cellFirst, uint32_t* __restrict__ cellIds, uint32_t* __restrict__ counters) {
    const uint32_t g = blockIdx.x * WG + threadIdx.x;
    if (g < kVoxGridWords) { cellFirst[g] = kNone; cellIds[g] = g; }
    if (g < 64u) counters[g] = 0u;
}

__global__ __launch_bounds__(WG) void k_voxel_mark(const uint32_t* __restrict__ vox, const uint4* __restrict__ recs, uint64_t n, uint32_t* __restrict__ cellFirst,
                                                   uint32_t* __restrict__ counters) {
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint4 r = recs[i];
    if (!voxel_in_range(r.x, r.y, r.z)) { atomicAdd(&counters[1], 1u); return; }
    const uint32_t g = voxel_grid_cell(r.x, r.y, r.z);
    if (vox[kVoxGridOff + g] != 0u) return;
    if (atomicMin(&cellFirst[g], (uint32_t)i) == kNone) atomicAdd(&counters[0], 1u);   // (one lane per cell sees ~0: the count is exact)
}

__global__ __launch_bounds__(WG) void k_voxel_number(uint32_t* __restrict__ vox, const uint32_t* __restrict__ sortedCells, uint32_t used, uint32_t nNew) {
    const uint32_t r = blockIdx.x * WG + threadIdx.x;
    if (r >= nNew) return;
    const uint32_t g = sortedCells[r];
    if (g < kVoxGridWords) vox[kVoxGridOff + g] = used + r;
}

__global__ __launch_bounds__(WG) void k_voxel_winner(const uint32_t* __restrict__ vox, const uint4* __restrict__ recs, uint64_t n, uint32_t* __restrict__ winner) {
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint4 r = recs[i];
    if (!voxel_in_range(r.x, r.y, r.z)) return;
    const uint32_t b = vox[kVoxGridOff + voxel_grid_cell(r.x, r.y, r.z)];
    if (b == 0u) return;   // (cannot happen after k_voxel_number; brick 0 is never written)
    atomicMax(&winner[(size_t)b * kVoxBrickWords + voxel_in_brick(r.x, r.y, r.z)], (uint32_t)i + 1u);
}

__global__ __launch_bounds__(WG) void k_voxel_store(uint32_t* __restrict__ vox, const uint4* __restrict__ recs, uint64_t n, uint32_t* __restrict__ winner) {
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint4 r = recs[i];
    if (!voxel_in_range(r.x, r.y, r.z)) return;
    const uint32_t b = vox[kVoxGridOff + voxel_grid_cell(r.x, r.y, r.z)];
    if (b == 0u) return;
    const size_t slot = (size_t)b * kVoxBrickWords + voxel_in_brick(r.x, r.y, r.z);
    // only the winner writes either word; the other records of the voxel read i' + 1 or 0, and neither is theirs
    if (winner[slot] == (uint32_t)i + 1u) { vox[kVoxBrickOff + slot] = r.w; winner[slot] = 0u; }
}

// UpdateTopGrid: lane ti = top cell x + 8 y + 64 z; a wave's 64 answers are two of the 16 words
__global__ __launch_bounds__(512) void k_voxel_top_grid(uint32_t* __restrict__ vox) {
    const uint32_t ti = threadIdx.x;
    const bool has = voxel_group_filled(vox + kVoxGridOff, ti);
    const unsigned long long m = __ballot(has);
    if ((ti & 63u) == 0u) { vox[ti >> 5] = (uint32_t)m; vox[(ti >> 5) + 1u] = (uint32_t)(m >> 32); }
}

__global__ __launch_bounds__(WG) void k_voxel_normals(const float4* __restrict__ instances, uint64_t nInst, const char* __restrict__ rays, uint32_t strideBytes, uint64_t n,
                                                      float4* __restrict__ out, uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    float4 N;
    if (!voxel_normal_record((const float4*)(rays + i * strideBytes), instances, nInst, &N)) atomicOr(status, kStatusVoxelNormal);
    out[i] = N;
}

// ---- voxelising a traced scene ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_voxelize_rays(VoxelizeArgs p, RayRec* __restrict__ rays, uint32_t* __restrict__ ids, uint32_t* __restrict__ hitNo) {
    const uint32_t id = blockIdx.x * WG + threadIdx.x;
    if (id >= kVoxelizeRays) return;
    const uint32_t a = id >> 16;
    float O[3];
    voxelize_origin(p, id, O);
    // the Ray constructor (tiny_bvh.h:695-703) for a unit axis: D as given, rD = tinybvh_safercp( D ) = 1 / 1e30, mask 0xFFFF, hit.t = 1e30
    RayRec r;
    r.O = make_float4(O[0], O[1], O[2], as_f32(0xFFFFu));
    r.D = make_float4(a == 0u ? 1.f : 0.f, a == 1u ? 1.f : 0.f, a == 2u ? 1.f : 0.f, as_f32(0u));
    r.rD = make_float4(a == 0u ? 1.f : kFar, a == 1u ? 1.f : kFar, a == 2u ? 1.f : kFar, as_f32(0u));
    r.hit = make_float4(1e30f, 0.f, 0.f, as_f32(0u));
    rays[id] = r; ids[id] = id; hitNo[id] = 0u;
}

__global__ __launch_bounds__(WG) void k_voxelize_step(VoxelizeArgs p, const RayRec* __restrict__ rays, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ hitNo,
                                                      const float4* __restrict__ out48, uint64_t n, RayRec* __restrict__ raysOut, uint32_t* __restrict__ idsOut,
                                                      uint32_t* __restrict__ hitNoOut, unsigned long long* __restrict__ keys, uint4* __restrict__ recs,
                                                      uint32_t* __restrict__ counters) {
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    RayRec r = rays[i];
    const float t = r.hit.x;
    if (t >= 10000.f) return;                                    // `if (ray.hit.t >= 10000) break` (240)
    const uint32_t id = ids[i], hits = hitNo[i], a = id >> 16;
    if (hits >= p.maxHits) { atomicAdd(&counters[2], 1u); return; }   // the stated deviation: the reference's loop has no cap
    const float Ix = __builtin_fmaf(r.D.x, t, r.O.x), Iy = __builtin_fmaf(r.D.y, t, r.O.y), Iz = __builtin_fmaf(r.D.z, t, r.O.z);
    const float4 sh = out48 ? out48[i * 3] : make_float4(0.f, 0.f, 0.f, 1.f);
    if (!(sh.w == 0.f)) {                                         // `if (alpha == 0) continue` (244)
        uint32_t P[3];
        voxelize_cell(p, id, a == 0u ? Ix : a == 1u ? Iy : Iz, P);
        const uint32_t v = out48 ? voxelize_value(sh.x, sh.y, sh.z) : p.color;
        const uint32_t slot = atomicAdd(&counters[1], 1u);
        recs[slot] = make_uint4(P[0], P[1], P[2], v);
        keys[slot] = ((unsigned long long)id << 32) | hits;
    }
    r.O = make_float4(__builtin_fmaf(r.D.x, 0.0001f, Ix), __builtin_fmaf(r.D.y, 0.0001f, Iy), __builtin_fmaf(r.D.z, 0.0001f, Iz), r.O.w);
    r.hit.x = 1e34f;                                             // (242; u, v, prim and hit.inst stay as the hit left them)
    const uint32_t live = atomicAdd(&counters[0], 1u);
    raysOut[live] = r; idsOut[live] = id; hitNoOut[live] = hits + 1u;
}

__global__ __launch_bounds__(WG) void k_voxelize_iota(uint32_t* __restrict__ order, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i < n) order[i] = (uint32_t)i;
}
__global__ __launch_bounds__(WG) void k_voxelize_gather(const uint4* __restrict__ recs, const uint32_t* __restrict__ order, uint4* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i < n) { const uint32_t j = order[i]; if (j < n) out[i] = recs[j]; }
}

inline uint32_t blocksFor(uint64_t n) { return (uint32_t)((n + WG - 1) / WG); }

}  // namespace

size_t voxel_edit_work_words(size_t* sortTempBytes) {
    size_t tmp = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)kVoxGridWords, 0, 32);
    *sortTempBytes = tmp;
    return 4 * (size_t)kVoxGridWords + 64 + (tmp + 3) / 4;
}

VoxelEditWork voxel_edit_work(uint32_t* base, size_t sortTempBytes) {
    VoxelEditWork w;
    w.cellFirst = base; w.cellIds = base + kVoxGridWords; w.sortedFirst = base + 2 * kVoxGridWords; w.sortedCells = base + 3 * kVoxGridWords;
    w.counters = base + 4 * kVoxGridWords;
    w.sortTemp = base + 4 * kVoxGridWords + 64;
    w.sortTempBytes = sortTempBytes;
    return w;
}

void launch_voxel_mark(const uint32_t* vox, const uint4* recs, uint64_t n, const VoxelEditWork& w, hipStream_t s) {
    hipLaunchKernelGGL(k_voxel_prep, dim3(kVoxGridWords / WG), dim3(WG), 0, s, w.cellFirst, w.cellIds, w.counters);
    hipLaunchKernelGGL(k_voxel_mark, dim3(blocksFor(n)), dim3(WG), 0, s, vox, recs, n, w.cellFirst, w.counters);
}

hipError_t launch_voxel_number(uint32_t* vox, const VoxelEditWork& w, uint32_t used, uint32_t nNew, hipStream_t s) {
    size_t tmp = w.sortTempBytes;
    const hipError_t e = hipcub::DeviceRadixSort::SortPairs(w.sortTemp, tmp, (const uint32_t*)w.cellFirst, w.sortedFirst, (const uint32_t*)w.cellIds, w.sortedCells,
                                                            (int)kVoxGridWords, 0, 32, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_voxel_number, dim3(blocksFor(nNew)), dim3(WG), 0, s, vox, w.sortedCells, used, nNew);
    return hipGetLastError();
}

void launch_voxel_winner(const uint32_t* vox, const uint4* recs, uint64_t n, uint32_t* winner, hipStream_t s) {
    hipLaunchKernelGGL(k_voxel_winner, dim3(blocksFor(n)), dim3(WG), 0, s, vox, recs, n, winner);
}

void launch_voxel_store(uint32_t* vox, const uint4* recs, uint64_t n, uint32_t* winner, hipStream_t s) {
    hipLaunchKernelGGL(k_voxel_store, dim3(blocksFor(n)), dim3(WG), 0, s, vox, recs, n, winner);
}

void launch_voxel_top_grid(uint32_t* vox, hipStream_t s) { hipLaunchKernelGGL(k_voxel_top_grid, dim3(1), dim3(512), 0, s, vox); }

void launch_voxelize_rays(const VoxelizeArgs& p, RayRec* rays, uint32_t* ids, uint32_t* hitNo, hipStream_t s) {
    hipLaunchKernelGGL(k_voxelize_rays, dim3(blocksFor(kVoxelizeRays)), dim3(WG), 0, s, p, rays, ids, hitNo);
}

void launch_voxelize_step(const VoxelizeArgs& p, const RayRec* rays, const uint32_t* ids, const uint32_t* hitNo, const float4* out48, uint64_t n, RayRec* raysOut,
                          uint32_t* idsOut, uint32_t* hitNoOut, unsigned long long* keys, uint4* recs, uint32_t* counters, hipStream_t s) {
    hipLaunchKernelGGL(k_voxelize_step, dim3(blocksFor(n)), dim3(WG), 0, s, p, rays, ids, hitNo, out48, n, raysOut, idsOut, hitNoOut, keys, recs, counters);
}

size_t voxelize_sort_temp_bytes(uint64_t n) {
    size_t tmp = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, 64);
    return tmp;
}

hipError_t launch_voxelize_sort(const unsigned long long* keys, unsigned long long* keysOut, uint32_t* order, uint32_t* orderOut, const uint4* recs, uint4* recsOut,
                                uint64_t n, void* temp, size_t tempBytes, hipStream_t s) {
    hipLaunchKernelGGL(k_voxelize_iota, dim3(blocksFor(n)), dim3(WG), 0, s, order, n);
    const hipError_t e = hipcub::DeviceRadixSort::SortPairs(temp, tempBytes, keys, keysOut, (const uint32_t*)order, orderOut, (int)n, 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_voxelize_gather, dim3(blocksFor(n)), dim3(WG), 0, s, recs, orderOut, recsOut, n);
    return hipGetLastError();
}

void launch_voxel_normals(const float4* instances, uint64_t nInst, const void* rays, uint32_t strideBytes, uint64_t n, float4* out, uint32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(k_voxel_normals, dim3(blocksFor(n)), dim3(WG), 0, s, instances, nInst, (const char*)rays, strideBytes, n, out, status);
}

}  // namespace tbvh
