// capi_voxel_edit.hip — editing a VOXELSET scene where it lies (include/tinybvh_amd.h: "editing a voxel set"): creation, capacity, the batched Set,
// UpdateTopGrid, the download, GetNormal for batches of hit records, and the scene-to-voxels loop (tbvh_voxelize_device).  The kernels are kernels_voxel_edit.hip, the rules voxel_edit.h, the CPU twins
// voxel_edit_host.cpp.
// The scene keeps ONE allocation in `nodes`: [top grid 16 | grid 32768 | bricks capacity x 512] uint32 words (capi_voxel.hip), nNodes = the used bricks.
// Growth is allocate, copy, zero the tail, swap; a TLAS over the set snapshots `nodes` in its BlasDesc table, so every TLAS over it is reclassified
// (which rewrites that table) before the old allocation goes.
#include "capi_internal.h"
#include "voxel_edit.h"

#include <algorithm>

using namespace tbvh;
using namespace tbvh_capi;

namespace {

uint64_t wordsFor(uint64_t bricks) { return (uint64_t)kVoxBrickOff + bricks * kVoxBrickWords; }
uint64_t capacityOf(const tbvh_scene* s) { return (s->nodes.count() * 4 - kVoxBrickOff) / kVoxBrickWords; }
uint32_t* wordsOf(const tbvh_scene* s) { return (uint32_t*)s->nodes.get(); }

int checkVoxelScene(const tbvh_scene* s, const char* who) {
    if (!s) return fail(TBVH_E_INVALID, "%s: null scene", who);
    if (s->layout != TBVH_LAYOUT_VOXELSET || s->isTlas || s->zombie) return fail(TBVH_E_INVALID, "%s: not a voxel set (layout %d)", who, s->layout);
    return 0;
}

// capacity >= bricks: a new allocation with the old contents and a zero tail, the TLASes over the set pointed at it, then the old one freed.  The winner
// words follow the capacity (all zero, as they are between calls).
int growTo(tbvh_scene* s, uint64_t bricks, const char* who) {
    tbvh_context* c = s->ctx;
    const uint64_t cap = capacityOf(s);
    if (bricks > kVoxMaxBricks) return fail(TBVH_E_FORMAT, "%s: %llu bricks: at most %llu", who, (unsigned long long)bricks, (unsigned long long)kVoxMaxBricks);
    if (bricks <= cap) return 0;
    DevBuf<float4> fresh;
    if (fresh.alloc(wordsFor(bricks) / 4) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: %llu bytes of device memory", who, (unsigned long long)(wordsFor(bricks) * 4)); }
    uint32_t* to = (uint32_t*)fresh.get();
    HIP_TRY(hipMemcpyAsync(to, wordsOf(s), wordsFor(cap) * 4, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(to + wordsFor(cap), 0, (bricks - cap) * kVoxBrickWords * 4, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // no query may still read the old arrays
    DevBuf<float4> old = std::move(s->nodes);
    s->nodes = std::move(fresh);
    s->voxWinner.reset();                       // (made again, for the new capacity, by the next Set)
    const int r = forEachTlasOver(s, reclassifyTlas);   // the descriptors are rewritten before the old arrays go
    if (r != 0) (void)old.release();            // (a failed refresh may have left a descriptor on the old arrays: leak them rather than dangle)
    return r;
}

int ensureEditScratch(tbvh_scene* s, const char* who) {
    tbvh_context* c = s->ctx;
    if (!s->voxWork) {
        size_t tmp = 0;
        const size_t words = voxel_edit_work_words(&tmp);
        if (s->voxWork.alloc(words) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: %llu bytes of device memory", who, (unsigned long long)(words * 4)); }
        s->voxSortTemp = tmp;
    }
    const uint64_t want = capacityOf(s) * kVoxBrickWords;
    if (s->voxWinner.count() != want) {
        if (s->voxWinner.alloc(want) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: %llu bytes of device memory", who, (unsigned long long)(want * 4)); }
        HIP_TRY(hipMemsetAsync(s->voxWinner, 0, want * 4, c->stream));
    }
    return 0;
}

int checkNormalsScene(tbvh_context* c, const tbvh_scene* s, const char* who) {
    if (!s) return 0;
    if (s->ctx != c) return fail(TBVH_E_INVALID, "%s: the scene belongs to another context", who);
    if (s->layout == TBVH_LAYOUT_VOXELSET && !s->isTlas) return 0;
    if (s->isTlas && s->layout != TBVH_LAYOUT_BVH_DOUBLE && s->tlas.nBlas && s->tlas.blasList[0]->layout == TBVH_LAYOUT_VOXELSET) return 0;
    return fail(TBVH_E_INVALID, "%s: a voxel set, a TLAS over voxel sets, or no scene (one set) is taken", who);
}

}  // namespace

extern "C" {

int tbvh_voxelset_create(tbvh_context* c, uint64_t brickCapacity, tbvh_scene** out) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_voxelset_create: null argument");
    if (brickCapacity == 0) brickCapacity = 1;
    if (brickCapacity > kVoxMaxBricks)
        return fail(TBVH_E_FORMAT, "tbvh_voxelset_create: %llu bricks: at most %llu", (unsigned long long)brickCapacity, (unsigned long long)kVoxMaxBricks);
    TBVH_ENTER(c);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_VOXELSET);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    static_assert(kVoxBrickOff % 4 == 0 && kVoxBrickWords % 4 == 0, "each part is a whole number of the 16-byte blocks `nodes` counts");
    if (s->nodes.alloc(wordsFor(brickCapacity) / 4) != hipSuccess) { (void)hipGetLastError(); tbvh_free_scene(s); return fail(TBVH_E_NOMEM, "tbvh_voxelset_create: out of device memory"); }
    if (hipMemsetAsync(s->nodes, 0, wordsFor(brickCapacity) * 4, c->stream) != hipSuccess) { tbvh_free_scene(s); return fail(TBVH_E_HIP, "tbvh_voxelset_create: clearing the set failed"); }
    s->nNodes = 1;   // freeBrickPtr: brick 0 is skipped
    *out = s;
    return 0;
}

int tbvh_voxelset_reserve(tbvh_scene* s, uint64_t nBricks) {
    if (int r = checkVoxelScene(s, "tbvh_voxelset_reserve")) return r;
    TBVH_ENTER(s->ctx);
    return growTo(s, nBricks, "tbvh_voxelset_reserve");
}

int tbvh_voxelset_capacity(tbvh_scene* s, uint64_t* capOut, uint64_t* usedOut) {
    if (int r = checkVoxelScene(s, "tbvh_voxelset_capacity")) return r;
    TBVH_LOCK(s->ctx);
    if (capOut) *capOut = capacityOf(s);
    if (usedOut) *usedOut = s->nNodes;
    return 0;
}

int tbvh_voxelset_set(tbvh_scene* s, const uint32_t* xyzv, uint64_t n, int onDevice) {
    if (int r = checkVoxelScene(s, "tbvh_voxelset_set")) return r;
    if (n == 0) return 0;
    if (!xyzv) return fail(TBVH_E_INVALID, "tbvh_voxelset_set: null records");
    if (n >> 31) return fail(TBVH_E_INVALID, "tbvh_voxelset_set: %llu records in one batch (fewer than 2^31)", (unsigned long long)n);
    if (onDevice && ((uintptr_t)xyzv & 15)) return fail(TBVH_E_INVALID, "tbvh_voxelset_set: a device record array must be 16-byte aligned");
    if (!onDevice)
        for (uint64_t i = 0; i < n; i++)
            if (!voxel_in_range(xyzv[i * 4], xyzv[i * 4 + 1], xyzv[i * 4 + 2]))
                return fail(TBVH_E_INVALID, "tbvh_voxelset_set: record %llu: voxel (%u, %u, %u) is outside the set's %u^3", (unsigned long long)i, xyzv[i * 4], xyzv[i * 4 + 1],
                            xyzv[i * 4 + 2], kVoxObjDim);
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    if (int r = ensureEditScratch(s, "tbvh_voxelset_set")) return r;
    const uint4* recs = (const uint4*)xyzv;
    if (!onDevice) {
        if (s->voxStage.reserve(n * 4) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "tbvh_voxelset_set: %llu bytes of device memory", (unsigned long long)(n * 16)); }
        HIP_TRY(hipMemcpyAsync(s->voxStage, xyzv, n * 16, hipMemcpyHostToDevice, c->stream));
        recs = (const uint4*)s->voxStage.get();
    }
    // TWO timed operations (tbvh_time_history): the mark pass with the one read-back, then everything that writes the set.  What lies between them — the
    // refusal, growth — is decided outside either, so no exit leaves an event pair open.
    HIP_TRY(timedBegin(c));
    const VoxelEditWork w = voxel_edit_work(s->voxWork, s->voxSortTemp);
    launch_voxel_mark(wordsOf(s), recs, n, w, c->stream);
    HIP_TRY(hipGetLastError());
    // the one read-back: how many grid cells get a brick, how many records are out of range.  Capacity is decided from it before anything is numbered.
    uint32_t counts[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(counts, w.counters, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(timedEnd(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t used = s->nNodes, nNew = counts[0], nBad = counts[1];
    if (nNew) {
        const uint64_t need = (uint64_t)used + nNew, cap = capacityOf(s);
        if (need > kVoxMaxBricks)
            return fail(TBVH_E_FORMAT, "tbvh_voxelset_set: the batch takes the set to %llu bricks: at most %llu (nothing was written)", (unsigned long long)need,
                        (unsigned long long)kVoxMaxBricks);
        if (need > cap) {   // the reference grows by a quarter (tiny_bvh.h:3796); by half here, and at least to what the batch needs
            uint64_t to = cap + (cap >> 1);
            if (to < need) to = need;
            if (to > kVoxMaxBricks) to = kVoxMaxBricks;
            if (int r = growTo(s, to, "tbvh_voxelset_set")) return r;
            if (int r = ensureEditScratch(s, "tbvh_voxelset_set")) return r;
        }
    }
    HIP_TRY(timedBegin(c));
    if (nNew) {
        HIP_TRY(hipMemsetAsync(wordsOf(s) + wordsFor(used), 0, (uint64_t)nNew * kVoxBrickWords * 4, c->stream));   // new bricks are zero before they are written
        HIP_TRY(launch_voxel_number(wordsOf(s), w, used, nNew, c->stream));
        s->nNodes = used + nNew;
    }
    launch_voxel_winner(wordsOf(s), recs, n, s->voxWinner, c->stream);
    launch_voxel_store(wordsOf(s), recs, n, s->voxWinner, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    if (!onDevice) HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's array may change on return (the staged copy has been read either way)
    if (nBad) return fail(TBVH_E_FORMAT, "tbvh_voxelset_set: %u of %llu device records have a coordinate beyond %u; they were skipped", nBad, (unsigned long long)n, kVoxObjDim - 1);
    return 0;
}

int tbvh_voxelset_update_top_grid(tbvh_scene* s) {
    if (int r = checkVoxelScene(s, "tbvh_voxelset_update_top_grid")) return r;
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    HIP_TRY(timedBegin(c));
    launch_voxel_top_grid(wordsOf(s), c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    return 0;
}

int tbvh_voxelset_download(tbvh_scene* s, uint32_t* grid, uint32_t* bricks, uint64_t capBricks, uint32_t* top, uint64_t* nBricks) {
    if (int r = checkVoxelScene(s, "tbvh_voxelset_download")) return r;
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    const uint64_t used = s->nNodes;
    if (nBricks) *nBricks = used;
    if (bricks && capBricks < used) return fail(TBVH_E_INVALID, "tbvh_voxelset_download: room for %llu bricks, the set uses %llu", (unsigned long long)capBricks, (unsigned long long)used);
    const uint32_t* base = wordsOf(s);
    if (top) HIP_TRY(hipMemcpyAsync(top, base, kVoxTopWords * 4, hipMemcpyDeviceToHost, c->stream));
    if (grid) HIP_TRY(hipMemcpyAsync(grid, base + kVoxGridOff, (size_t)kVoxGridWords * 4, hipMemcpyDeviceToHost, c->stream));
    if (bricks) HIP_TRY(hipMemcpyAsync(bricks, base + kVoxBrickOff, used * kVoxBrickWords * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// tiny_bvh_foliage.cpp:222-258 in rounds: trace -> shade -> step (kernels_voxel_edit.hip), then the records in loop order through the batched Set
int tbvh_voxelize_device(tbvh_scene* scene, tbvh_shading* sh, const tbvh_voxelize_params* prm, tbvh_scene* vs, tbvh_voxelize_stats* stats) {
    const char* who = "tbvh_voxelize_device";
    if (!scene || !prm || !vs) return fail(TBVH_E_INVALID, "%s: null argument", who);
    if (int r = checkVoxelScene(vs, who)) return r;
    TBVH_REFUSE_DOUBLE(scene, who);
    TBVH_REFUSE_VOXEL(scene, who);
    TBVH_REFUSE_CUSTOM(scene, who);
    if (scene->ctx != vs->ctx) return fail(TBVH_E_INVALID, "%s: the scene and the voxel set belong to different contexts", who);
    if (scene->isTlas && (scene->tlas.blasSpheres || (scene->tlas.nBlas && scene->tlas.blasList[0]->layout == TBVH_LAYOUT_VOXELSET)))
        return fail(TBVH_E_INVALID, "%s: a TLAS over triangle BLASes is taken; this one holds sphere or voxel BLASes", who);
    VoxelizeArgs a;
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(prm->bmin[k]) || !std::isfinite(prm->ext[k]) || !(prm->ext[k] > 0)) return fail(TBVH_E_INVALID, "%s: bmin[%d] = %g, ext[%d] = %g", who, k, prm->bmin[k], k, prm->ext[k]);
        a.bmin[k] = prm->bmin[k];
        a.reciExt[k] = 1.0f / prm->ext[k];   // `float reciExt = 1.0f / ext[a]` (226)
    }
    if (!std::isfinite(prm->maxSize)) return fail(TBVH_E_INVALID, "%s: maxSize = %g", who, prm->maxSize);
    a.maxSize = prm->maxSize; a.color = prm->color; a.maxHits = prm->max_hits_per_ray ? prm->max_hits_per_ray : 4096u;
    tbvh_context* c = vs->ctx;
    TBVH_ENTER(c);
    // two sets of ray arrays (a round reads one and compacts into the other), the shading records, three counters, and records + keys that grow
    const uint64_t nRays = kVoxelizeRays;
    DevBuf<RayRec> rays[2];
    DevBuf<uint32_t> ids[2], hitNo[2], counters;
    DevBuf<float4> out48;
    DevBuf<uint4> recs;
    DevBuf<unsigned long long> keys;
    uint64_t cap = 2 * nRays;
    bool ok = counters.alloc(4) == hipSuccess && recs.alloc(cap) == hipSuccess && keys.alloc(cap) == hipSuccess && (!sh || out48.alloc(nRays * 3) == hipSuccess);
    for (int k = 0; k < 2 && ok; k++) ok = rays[k].alloc(nRays) == hipSuccess && ids[k].alloc(nRays) == hipSuccess && hitNo[k].alloc(nRays) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: out of device memory", who); }
    HIP_TRY(hipMemsetAsync(counters, 0, 16, c->stream));
    launch_voxelize_rays(a, rays[0], ids[0], hitNo[0], c->stream);
    HIP_TRY(hipGetLastError());
    uint64_t live = nRays, total = 0, cut = 0;
    uint32_t rounds = 0;
    int cur = 0;
    while (live) {
        if (total + live > cap) {   // room for a record per live ray: a larger pair of arrays with what the rounds so far recorded
            const uint64_t to = std::max(cap * 2, total + live);
            DevBuf<uint4> r2;
            DevBuf<unsigned long long> k2;
            if (r2.alloc(to) != hipSuccess || k2.alloc(to) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: %llu records: out of device memory", who, (unsigned long long)to); }
            HIP_TRY(hipMemcpyAsync(r2, recs, total * 16, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(k2, keys, total * 8, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            recs = std::move(r2); keys = std::move(k2); cap = to;
        }
        if (int r = launchQuery(scene, rays[cur], live, nullptr)) return r;
        rounds++;
        if (sh) if (int r = tbvh_shade_hits_device(sh, scene, rays[cur], live, 64, out48)) return r;
        HIP_TRY(hipMemsetAsync(counters, 0, 4, c->stream));
        HIP_TRY(timedBegin(c));   // (a timed operation of its own, as the trace and the shading are: tools/voxel_edit_bench.py reads the stages apart)
        launch_voxelize_step(a, rays[cur], ids[cur], hitNo[cur], sh ? out48.get() : nullptr, live, rays[cur ^ 1], ids[cur ^ 1], hitNo[cur ^ 1], keys, recs, counters, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(timedEnd(c));
        uint32_t got[3] = {0, 0, 0};   // the round's one read-back: live rays of the next round, records so far, rays cut so far
        HIP_TRY(hipMemcpyAsync(got, counters, 12, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        live = got[0]; total = got[1]; cut = got[2];
        cur ^= 1;
    }
    if (int r = checkStatus(c)) return r;   // (a traversal stack overflow, a hit the shading table does not cover)
    if (total) {
        DevBuf<uint4> sorted;
        DevBuf<unsigned long long> keysOut;
        DevBuf<uint32_t> order, orderOut;
        DevBuf<void> temp;
        const size_t tempBytes = voxelize_sort_temp_bytes(total);
        if (sorted.alloc(total) != hipSuccess || keysOut.alloc(total) != hipSuccess || order.alloc(total) != hipSuccess || orderOut.alloc(total) != hipSuccess ||
            temp.alloc(tempBytes ? tempBytes : 16) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: sorting %llu records: out of device memory", who, (unsigned long long)total); }
        HIP_TRY(timedBegin(c));
        HIP_TRY(launch_voxelize_sort(keys, keysOut, order, orderOut, recs, sorted, total, temp, tempBytes, c->stream));
        HIP_TRY(timedEnd(c));
        if (int r = tbvh_voxelset_set(vs, (const uint32_t*)sorted.get(), total, 1)) return r;
        HIP_TRY(hipStreamSynchronize(c->stream));   // (the sorted records go with this scope)
    }
    if (int r = tbvh_voxelset_update_top_grid(vs)) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (stats) { stats->rounds = rounds; stats->reserved = 0; stats->records = total; stats->rays_cut = cut; stats->bricks = vs->nNodes; }
    return 0;
}

int tbvh_voxel_normals_device(tbvh_context* c, tbvh_scene* s, const void* dRays, uint32_t strideBytes, uint64_t n, void* dNormals) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_voxel_normals_device: null context");
    if (int r = checkNormalsScene(c, s, "tbvh_voxel_normals_device")) return r;
    if (strideBytes < 64 || (strideBytes & 15)) return fail(TBVH_E_INVALID, "tbvh_voxel_normals_device: a record stride of %u bytes (64 or more, a multiple of 16)", strideBytes);
    if (n && (!dRays || !dNormals)) return fail(TBVH_E_INVALID, "tbvh_voxel_normals_device: null records or output");
    if (((uintptr_t)dRays | (uintptr_t)dNormals) & 15) return fail(TBVH_E_INVALID, "tbvh_voxel_normals_device: misaligned records or output (16 bytes)");
    TBVH_ENTER(c);
    if (!n) return 0;
    const bool tlas = s && s->isTlas;
    HIP_TRY(timedBegin(c));
    launch_voxel_normals(tlas ? s->tlas.instances.get() : nullptr, tlas ? s->tlas.nInst : 0, dRays, strideBytes, n, (float4*)dNormals, c->status, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    return 0;
}

int tbvh_voxel_normals(tbvh_context* c, tbvh_scene* s, const void* rays, uint32_t strideBytes, uint64_t n, void* normals) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_voxel_normals: null context");
    if (int r = checkNormalsScene(c, s, "tbvh_voxel_normals")) return r;
    if (strideBytes < 64 || (strideBytes & 3)) return fail(TBVH_E_INVALID, "tbvh_voxel_normals: a record stride of %u bytes (64 or more, a multiple of 4)", strideBytes);
    if (n && (!rays || !normals)) return fail(TBVH_E_INVALID, "tbvh_voxel_normals: null records or output");
    if (((uintptr_t)rays | (uintptr_t)normals) & 3) return fail(TBVH_E_INVALID, "tbvh_voxel_normals: misaligned records or output (4 bytes)");
    TBVH_ENTER(c);
    if (!n) return 0;
    // the 64-byte prefixes go up packed, the normals come back; both staging areas live for the call
    DevBuf<void> dRays, dOut;
    if (dRays.alloc(n * 64) != hipSuccess || dOut.alloc(n * 16) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "tbvh_voxel_normals: %llu bytes of device memory", (unsigned long long)(n * 80)); }
    HIP_TRY(hipMemcpy2DAsync(dRays, 64, rays, strideBytes, 64, n, hipMemcpyHostToDevice, c->stream));
    int r = tbvh_voxel_normals_device(c, s, dRays, 64, n, dOut);
    if (!r && hipMemcpyAsync(normals, dOut, n * 16, hipMemcpyDeviceToHost, c->stream) != hipSuccess) r = fail(TBVH_E_HIP, "tbvh_voxel_normals: copying the normals back failed: %s", hipGetErrorString(hipGetLastError()));
    const int st = checkStatus(c);   // (synchronizes: the staging areas may go)
    return r ? r : st;
}

}  // extern "C"
