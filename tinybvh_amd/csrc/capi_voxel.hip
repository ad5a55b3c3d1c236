// capi_voxel.hip — VoxelSet scenes (tiny_bvh.h:988-1030, 3772-4158): upload with validation and the host builder behind
// tbvh_host_build_voxelset.  The kernels are kernels_voxel.hip; queries reach them through launchQuery (capi_query.hip), TLASes over voxel sets
// through tbvh_upload_tlas (capi_scene.hip).
// A VOXELSET scene keeps ONE device allocation in `nodes`: [top grid 16 | grid 32768 | bricks n_bricks x 512] uint32 words, which is also
// what a TLAS's BlasDesc::nodes points at.  tbvh_free_scene frees it like any scene's nodes.
#include "capi_internal.h"
#include "voxel_edit.h"

using namespace tbvh;
using namespace tbvh_capi;

namespace {

constexpr uint32_t kObjDim = kVoxObjDim;   // VoxelSet::objectDim = 256 (tiny_bvh.h:1008-1022); the dimensions are voxel_edit.h's
constexpr uint64_t kGridWords = kVoxGridWords, kBrickWords = kVoxBrickWords, kTopWords = kVoxTopWords, kMaxBricks = kVoxMaxBricks;

// VoxelSet::Set (tiny_bvh.h:3786-3807) and UpdateTopGrid (3809-3827): voxel_edit.h, shared with the editing entry points (capi_voxel_edit.hip,
// voxel_edit_host.cpp)
void setVoxel(tbvh_hostbvh* h, uint32_t x, uint32_t y, uint32_t z, uint32_t v) { voxel_set_host(h->vgrid, h->vbricks, x, y, z, v); }
void updateTopGrid(tbvh_hostbvh* h) {
    h->vtop.assign(kTopWords, 0u);
    voxel_update_top_grid_host(h->vgrid.data(), h->vtop.data());
}

}  // namespace

extern "C" {

int tbvh_upload_voxelset(tbvh_context* c, const uint32_t* grid, const uint32_t* bricks, uint64_t nBricks, const uint32_t* top, tbvh_scene** out) {
    if (!c || !grid || !bricks || !top || !out) return fail(TBVH_E_INVALID, "tbvh_upload_voxelset: null argument");
    if (nBricks == 0) return fail(TBVH_E_FORMAT, "tbvh_upload_voxelset: n_bricks = 0 (brick 0, the empty one, is part of the pool)");
    if (nBricks > kMaxBricks) return fail(TBVH_E_FORMAT, "tbvh_upload_voxelset: %llu bricks: at most %llu", (unsigned long long)nBricks, (unsigned long long)kMaxBricks);
    for (uint64_t i = 0; i < kGridWords; i++)
        if (grid[i] >= nBricks)
            return fail(TBVH_E_FORMAT, "tbvh_upload_voxelset: grid[%llu] = %u >= n_bricks = %llu", (unsigned long long)i, grid[i], (unsigned long long)nBricks);
    TBVH_ENTER(c);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_VOXELSET);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    static_assert(kTopWords % 4 == 0 && kGridWords % 4 == 0 && kBrickWords % 4 == 0, "each part is a whole number of the 16-byte blocks `nodes` counts");
    const uint64_t words = kTopWords + kGridWords + nBricks * kBrickWords;
    if (s->nodes.alloc(words / 4) != hipSuccess) { tbvh_free_scene(s); return fail(TBVH_E_NOMEM, "tbvh_upload_voxelset: out of device memory"); }
    uint32_t* base = (uint32_t*)s->nodes.get();
    if (hipMemcpyAsync(base, top, kTopWords * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(base + kTopWords, grid, kGridWords * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(base + kTopWords + kGridWords, bricks, nBricks * kBrickWords * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        tbvh_free_scene(s);
        return fail(TBVH_E_HIP, "tbvh_upload_voxelset: copy to the device failed");
    }
    s->nNodes = (uint32_t)nBricks;
    *out = s;
    return 0;
}

int tbvh_host_build_voxelset(const uint32_t* values, uint32_t nx, uint32_t ny, uint32_t nz, tbvh_hostbvh** out) {
    if (!values || !out || !nx || !ny || !nz) return fail(TBVH_E_INVALID, "tbvh_host_build_voxelset: null/empty argument");
    if (nx > kObjDim || ny > kObjDim || nz > kObjDim)
        return fail(TBVH_E_INVALID, "tbvh_host_build_voxelset: extent %u x %u x %u beyond the object's %u^3 voxels", nx, ny, nz, kObjDim);
    tbvh_hostbvh* h = new (std::nothrow) tbvh_hostbvh;
    if (!h) return fail(TBVH_E_NOMEM, "out of host memory");
    h->layout = TBVH_LAYOUT_VOXELSET;
    try {
        h->vgrid.assign(kGridWords, 0u);
        h->vbricks.assign(kBrickWords, 0u);   // brick 0: never written
        for (uint32_t x = 0; x < nx; x++) for (uint32_t y = 0; y < ny; y++) for (uint32_t z = 0; z < nz; z++) {   // tiny_bvh_voxel.cpp's loop order
            const uint32_t v = values[x + (size_t)y * nx + (size_t)z * nx * ny];
            if (v) setVoxel(h, x, y, z, v);
        }
        updateTopGrid(h);
    } catch (const std::bad_alloc&) {
        delete h;
        return fail(TBVH_E_NOMEM, "out of host memory while building");
    }
    *out = h;
    return 0;
}

// ---- the CPU twins of the editing calls (capi_voxel_edit.hip): the reference's constructor, Set per record in turn, UpdateTopGrid ------------------
int tbvh_host_voxelset_create(tbvh_hostbvh** out) {
    if (!out) return fail(TBVH_E_INVALID, "tbvh_host_voxelset_create: null argument");
    tbvh_hostbvh* h = new (std::nothrow) tbvh_hostbvh;
    if (!h) return fail(TBVH_E_NOMEM, "out of host memory");
    h->layout = TBVH_LAYOUT_VOXELSET;
    try {
        h->vgrid.assign(kGridWords, 0u);
        h->vbricks.assign(kBrickWords, 0u);   // brick 0: never written (freeBrickPtr = 1)
        h->vtop.assign(kTopWords, 0u);
    } catch (const std::bad_alloc&) {
        delete h;
        return fail(TBVH_E_NOMEM, "out of host memory");
    }
    *out = h;
    return 0;
}

int tbvh_host_voxelset_set(tbvh_hostbvh* h, const uint32_t* xyzv, uint64_t n) {
    if (!h || h->layout != TBVH_LAYOUT_VOXELSET) return fail(TBVH_E_INVALID, "tbvh_host_voxelset_set: not a voxel set");
    return voxel_host_set_records(h->vgrid, h->vbricks, xyzv, n);   // (voxel_edit_host.cpp: the refusals first, then setVoxel's Set per record)
}

int tbvh_host_voxelset_update_top_grid(tbvh_hostbvh* h) {
    if (!h || h->layout != TBVH_LAYOUT_VOXELSET) return fail(TBVH_E_INVALID, "tbvh_host_voxelset_update_top_grid: not a voxel set");
    updateTopGrid(h);
    return 0;
}

int tbvh_upload_voxelset_dense(tbvh_context* c, const uint32_t* values, uint32_t nx, uint32_t ny, uint32_t nz, tbvh_scene** out) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_upload_voxelset_dense: null argument");
    tbvh_hostbvh* h = nullptr;
    if (int r = tbvh_host_build_voxelset(values, nx, ny, nz, &h)) return r;
    const int r = tbvh_upload_voxelset(c, h->vgrid.data(), h->vbricks.data(), h->vbricks.size() / kBrickWords, h->vtop.data(), out);
    delete h;
    return r;
}

}  // extern "C"
