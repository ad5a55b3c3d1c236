// voxel_edit_host.cpp — the CPU twins of the voxel editing calls (include/tinybvh_amd.h: "editing a voxel set"): the batched Set over a host set's arrays
// (tbvh_host_voxelset_set, capi_voxel.hip, is this over a tbvh_hostbvh) and GetNormal over host records, through voxel_edit.h — the header the kernels
// compile.  Plain C++ that needs voxel_edit.h, the public header and the library's error helper only, so that it can also be compiled on its own.  No
// context, no device.  Built -ffp-contract=off like the rest.
#include <string.h>

#include <new>

#include "../../include/tinybvh_amd.h"
#include "voxel_edit.h"

namespace tbvh_capi {
int fail(int code, const char* fmt, ...);   // (capi_context.hip) sets tbvh_last_error() of the calling thread, returns code
}
using namespace tbvh;
using tbvh_capi::fail;

namespace tbvh {

int voxel_host_set_records(std::vector<uint32_t>& grid, std::vector<uint32_t>& bricks, const uint32_t* xyzv, uint64_t n) {
    if (n == 0) return 0;
    if (!xyzv) return fail(TBVH_E_INVALID, "tbvh_host_voxelset_set: null records");
    if (n >> 31) return fail(TBVH_E_INVALID, "tbvh_host_voxelset_set: %llu records in one batch (fewer than 2^31)", (unsigned long long)n);
    uint64_t fresh = 0;   // checked before anything is touched: the coordinates, and the bricks the batch adds
    std::vector<uint8_t> seen(kVoxGridWords, 0);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t x = xyzv[i * 4], y = xyzv[i * 4 + 1], z = xyzv[i * 4 + 2];
        if (!voxel_in_range(x, y, z))
            return fail(TBVH_E_INVALID, "tbvh_host_voxelset_set: record %llu: voxel (%u, %u, %u) is outside the set's %u^3", (unsigned long long)i, x, y, z, kVoxObjDim);
        const uint32_t g = voxel_grid_cell(x, y, z);
        if (!grid[g] && !seen[g]) { seen[g] = 1; fresh++; }
    }
    const uint64_t need = bricks.size() / kVoxBrickWords + fresh;
    if (need > kVoxMaxBricks)
        return fail(TBVH_E_FORMAT, "tbvh_host_voxelset_set: the batch takes the set to %llu bricks: at most %llu (nothing was written)", (unsigned long long)need,
                    (unsigned long long)kVoxMaxBricks);
    try {
        bricks.reserve(need * kVoxBrickWords);
        for (uint64_t i = 0; i < n; i++) voxel_set_host(grid, bricks, xyzv[i * 4], xyzv[i * 4 + 1], xyzv[i * 4 + 2], xyzv[i * 4 + 3]);
    } catch (const std::bad_alloc&) {
        return fail(TBVH_E_NOMEM, "tbvh_host_voxelset_set: out of host memory");
    }
    return 0;
}

}  // namespace tbvh

extern "C" {

int tbvh_host_voxel_normals(const void* instances192, uint64_t nInst, const void* rays, uint32_t strideBytes, uint64_t n, void* normals16) {
    if (strideBytes < 64 || (strideBytes & 3)) return fail(TBVH_E_INVALID, "tbvh_host_voxel_normals: a record stride of %u bytes (64 or more, a multiple of 4)", strideBytes);
    if (n && (!rays || !normals16)) return fail(TBVH_E_INVALID, "tbvh_host_voxel_normals: null records or output");
    if (((uintptr_t)rays | (uintptr_t)normals16 | (uintptr_t)instances192) & 3) return fail(TBVH_E_INVALID, "tbvh_host_voxel_normals: misaligned records, instances or output (4 bytes)");
    if (instances192 && nInst == 0) return fail(TBVH_E_INVALID, "tbvh_host_voxel_normals: an instance array without instances");
    bool ok = true;
    for (uint64_t i = 0; i < n; i++) {
        float4 rec[4], inst[12] = {}, N = make_float4(0.f, 0.f, 0.f, 0.f);
        memcpy(rec, (const char*)rays + i * strideBytes, 64);
        uint32_t hitInst;
        memcpy(&hitInst, &rec[2].w, 4);
        if (!instances192) ok &= voxel_normal_record(rec, nullptr, 0, &N);
        else if (hitInst >= nInst && rec[3].x < 1e30f) ok = false;   // (zeros; a miss's hit.inst is not looked at, as on the device)
        else {   // the one instance the hit names, copied out as instance 0: the caller's array need not be 16-byte aligned
            const uint32_t zero = 0;
            if (rec[3].x < 1e30f) memcpy(inst, (const char*)instances192 + (size_t)hitInst * 192, 192);
            memcpy(&rec[2].w, &zero, 4);
            ok &= voxel_normal_record(rec, inst, 1, &N);
        }
        memcpy((char*)normals16 + i * 16, &N, 16);
    }
    return ok ? 0 : fail(TBVH_E_FORMAT, "tbvh_host_voxel_normals: a hit record's instance index is not an instance (that record got zeros)");
}

}  // extern "C"
