// capi_scene.hip — scenes: uploads and their validation, in-place updates, device conversion / build / refit, TLAS upload, classification and rebuild,
// opacity maps, schedule hints.  The copies the library derives from a scene are capi_copies.hip's: this file reaches them through capi_internal.h's functions.
#include "capi_internal.h"
#include "sahbuild.h"

using namespace tbvh;
using namespace tbvh_capi;

namespace tbvh_capi {
tbvh_scene* newScene(tbvh_context* c, int layout) {
    tbvh_scene* s = new (std::nothrow) tbvh_scene;
    if (!s) return nullptr;
    s->ctx = c; s->layout = layout;
    c->scenes.push_back(s);
    return s;
}

// ---- device refit (tbvh_refit / tbvh_refit_mesh below) ----------------------------------------------------------------------------------
// the refit itself: src is device-resident (the caller's arrays, the scene's vertex staging buffer, the scene's held index buffer)
int refitDeviceSource(tbvh_scene* s, const MeshSrc& src) {
    tbvh_context* c = s->ctx;
    if (s->layout == TBVH_LAYOUT_BVH4_GPU) {
        // node list per level, child-box hand-over area: sized for the most nodes the stream can hold (4 blocks each)
        const uint32_t capNodes = (uint32_t)(s->nNodeBlocks / 4 + 1);
        if (!s->refitScratch) HIP_TRY(s->refitScratch.alloc((size_t)capNodes * (16 + 128) + 256));
        char* base = (char*)s->refitScratch.get();
        uint32_t* counter = (uint32_t*)base;
        void* items = base + 256;
        float4* childBox = (float4*)(base + 256 + (size_t)capNodes * 16);
        HIP_TRY(timedBegin(c));
        HIP_TRY(run_refit_bvh4(s->nodes, s->nNodeBlocks, src, items, capNodes, counter, childBox, s->b4Levels, c->status, c->stream));
        HIP_TRY(timedEnd(c));
        return refitCopies(s, src);   // the 8-wide copy follows
    }
    if (s->layout != TBVH_LAYOUT_CWBVH && s->layout != TBVH_LAYOUT_BVH_GPU)
        return fail(TBVH_E_INVALID, "tbvh_refit: layout %d is not refittable", s->layout);
    const uint32_t nNodes = (uint32_t)(s->layout == TBVH_LAYOUT_CWBVH ? s->nNodeBlocks / 5 : s->nNodeBlocks / 4);
    const uint64_t nRecords = s->nTriBlocks / 3;
    if (!s->refitScratch) HIP_TRY(s->refitScratch.alloc(refit_scratch_bytes(s->layout, nNodes)));
    HIP_TRY(timedBegin(c));
    HIP_TRY(launch_refit(s->layout, s->nodes, nNodes, s->tris, nRecords, src, s->refitScratch, c->status, c->stream));
    HIP_TRY(timedEnd(c));
    if (int r = rederiveCwbvhLayouts(s)) return r;   // the padded / hybrid nodes and the 64-byte triangle records would be stale now
    return refitCopies(s, src);                      // the 8-wide and the 4-wide copy follow
}
}  // namespace tbvh_capi

extern "C" {

// ---- uploads ---------------------------------------------------------------------------

// What a BVH_GPU upload and an in-place update share (skipped when e comes in as an error): the blob's nodes go into s->nodes, its primIdx names triangles,
// whose vertices the gather finds through the mesh (flat: 3 float4 per triangle) and writes to s->tris, an indexed mesh leaves its indices with the scene
// (counted in s->bytes: set before); synchronous.  e: the first HIP error — the caller words it and cleans up —, r: keepMeshIndices' code; general: the gather
// read through indices or a stride, so checkStatus is due (device-resident indices: the gather reports an index that is not a vertex)
struct BvhGpuFill { hipError_t e; int r; bool indexed, general; };
static BvhGpuFill fillBvhGpu(tbvh_scene* s, hipError_t e, const void* nodes64, uint64_t nNodes, const uint32_t* primIdx, uint64_t nIdx, const tbvh_mesh& mesh) {
    tbvh_context* c = s->ctx;
    DevBuf<uint32_t> dIdx;
    DeviceMesh dm;
    if (e == hipSuccess) e = dIdx.alloc(nIdx ? nIdx : 1);
    if (e == hipSuccess && stageMesh(c, mesh, dm)) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemcpyAsync(s->nodes, nodes64, nNodes * 64, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dIdx, primIdx, nIdx * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nIdx) { launch_gather_tris(dIdx, dm.src, s->tris, nIdx, c->status, c->stream); e = hipGetLastError(); }
    int r = 0;
    if (e == hipSuccess && dm.src.indices) r = keepMeshIndices(s, dm.src);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return {e, r, dm.src.indices != nullptr, dm.src.general()};
}

static int uploadBvhGpuImpl(tbvh_context* c, const void* nodes64, uint64_t nNodes, const uint32_t* primIdx, uint64_t nIdx, const tbvh_mesh& mesh, tbvh_scene** out) {
    if (const char* why = validate_bvh_gpu((const NodeAL*)nodes64, nNodes, nIdx)) return fail(why == kValidateNoMemory ? TBVH_E_NOMEM : TBVH_E_FORMAT, "%s", why);
    TBVH_ENTER(c);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_BVH_GPU);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    hipError_t e = s->nodes.alloc(nNodes * 4);
    if (e == hipSuccess) e = s->tris.alloc((nIdx ? nIdx : 1) * 3);
    s->nNodeBlocks = nNodes * 4; s->nTriBlocks = nIdx * 3;
    s->capNodeBlocks = s->nNodeBlocks; s->capTriBlocks = s->nTriBlocks;
    s->bytes = nNodes * 64 + nIdx * 48;
    const BvhGpuFill f = fillBvhGpu(s, e, nodes64, nNodes, primIdx, nIdx, mesh);
    if (f.e != hipSuccess) { tbvh_free_scene(s); return fail(TBVH_E_HIP, "BVH_GPU upload failed: %s", hipGetErrorString(f.e)); }
    int r = f.r;
    if (!r && f.general) r = checkStatus(c);
    if (r) { tbvh_free_scene(s); return r; }
    *out = s;
    return 0;
}

int tbvh_upload_bvh_gpu(tbvh_context* c, const void* nodes64, uint64_t nNodes, const uint32_t* primIdx, uint64_t nIdx,
                        const void* verts16, uint64_t nTris, tbvh_scene** out) {
    if (!c || !nodes64 || !primIdx || !verts16 || !out || nNodes == 0) return fail(TBVH_E_INVALID, "tbvh_upload_bvh_gpu: null/empty argument");
    return uploadBvhGpuImpl(c, nodes64, nNodes, primIdx, nIdx, flatMesh(verts16, nTris, 0), out);
}

int tbvh_upload_bvh_gpu_mesh(tbvh_context* c, const void* nodes64, uint64_t nNodes, const uint32_t* primIdx, uint64_t nIdx, const tbvh_mesh* mesh, tbvh_scene** out) {
    if (!c || !nodes64 || !primIdx || !out || nNodes == 0) return fail(TBVH_E_INVALID, "tbvh_upload_bvh_gpu_mesh: null/empty argument");
    if (int r = checkMesh(mesh, "tbvh_upload_bvh_gpu_mesh")) return r;
    return uploadBvhGpuImpl(c, nodes64, nNodes, primIdx, nIdx, *mesh, out);
}

int tbvh_upload_bvh4_gpu(tbvh_context* c, const void* blocks16, uint64_t nBlocks, tbvh_scene** out) {
    if (!c || !blocks16 || !out || nBlocks < 4) return fail(TBVH_E_INVALID, "tbvh_upload_bvh4_gpu: null/empty argument");
    if (const char* why = validate_bvh4_gpu((const Vec4*)blocks16, nBlocks)) return fail(why == kValidateNoMemory ? TBVH_E_NOMEM : TBVH_E_FORMAT, "%s", why);
    TBVH_ENTER(c);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_BVH4_GPU);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    hipError_t e = s->nodes.alloc(nBlocks);
    if (e == hipSuccess) e = hipMemcpyAsync(s->nodes, blocks16, nBlocks * 16, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { tbvh_free_scene(s); return fail(TBVH_E_HIP, "BVH4_GPU upload failed: %s", hipGetErrorString(e)); }
    s->nNodeBlocks = nBlocks; s->capNodeBlocks = nBlocks; s->bytes = nBlocks * 16;
    *out = s;
    return 0;
}

int tbvh_upload_cwbvh(tbvh_context* c, const void* nodes16, uint64_t nNodeBlocks, const void* tris16, uint64_t nTriBlocks,
                      tbvh_scene** out) {
    if (!c || !nodes16 || !out || nNodeBlocks < 5 || (nTriBlocks && !tris16)) return fail(TBVH_E_INVALID, "tbvh_upload_cwbvh: null/empty argument");
    if (nNodeBlocks % 5) return fail(TBVH_E_FORMAT, "CWBVH node blocks (%llu) not a multiple of 5", (unsigned long long)nNodeBlocks);
    if (nNodeBlocks >> 32) return fail(TBVH_E_FORMAT, "CWBVH node blocks (%llu) beyond the layout's 32-bit block index", (unsigned long long)nNodeBlocks);   // (cw_load_node: 32-bit float4 offsets)
    if (const char* why = validate_cwbvh((const Vec4*)nodes16, nNodeBlocks / 5, nTriBlocks)) return fail(why == kValidateNoMemory ? TBVH_E_NOMEM : TBVH_E_FORMAT, "%s", why);
    TBVH_ENTER(c);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_CWBVH);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    hipError_t e = s->nodes.alloc(nNodeBlocks);
    if (e == hipSuccess) e = s->tris.alloc(nTriBlocks ? nTriBlocks : 1);
    if (e == hipSuccess) e = hipMemcpyAsync(s->nodes, nodes16, nNodeBlocks * 16, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nTriBlocks) e = hipMemcpyAsync(s->tris, tris16, nTriBlocks * 16, hipMemcpyHostToDevice, c->stream);
    s->nNodes = (uint32_t)(nNodeBlocks / 5);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { tbvh_free_scene(s); return fail(TBVH_E_HIP, "CWBVH upload failed: %s", hipGetErrorString(e)); }
    s->nNodeBlocks = nNodeBlocks; s->nTriBlocks = nTriBlocks;
    s->capNodeBlocks = nNodeBlocks; s->capTriBlocks = nTriBlocks ? nTriBlocks : 1;
    s->topoHash = cwbvhTopologyHash((const Vec4*)nodes16, s->nNodes);
    s->bytes = (nNodeBlocks + nTriBlocks) * 16;
    if (int r = resetCwbvhLayouts(s)) { tbvh_free_scene(s); return r; }
    *out = s;
    return 0;
}

namespace {
// (re)build the wide TLAS(es) from the BVH_GPU nodes on the device — 8-wide in the BVH8_CWBVH node format, 4-wide in the BVH4_GPU one, whichever the
// two-level kernels of this TLAS's closest-hit and any-hit queries walk; asynchronous on the context's stream
// the scratch area the two wide builds share holds what this TLAS needs
int reserveTlasWideScratch(tbvh_scene* s) {
    HIP_TRY(s->tlas4Scratch.reserve(tlas_wide_scratch_bytes(s->nTlasNodes, s->nInst)));
    return 0;
}

int buildTlasWide8(tbvh_scene* s) {
    tbvh_context* c = s->ctx;
    const uint64_t cap = tlas8_cap_nodes(s->nTlasNodes, s->nInst);
    if (cap > 0x00ffffffull) {   // wide-node indices share a word with 8 flag bits in places: the flat loop serves larger TLASes — and a wide
        // TLAS left from an earlier, smaller upload must not be traversed in its place (launchQuery keys on the pointer)
        s->tlas8.reset(); s->tlas8Refs.reset();
        return 0;
    }
    if (cap * 5 > s->tlas8.count()) {
        // both go before either is made again, and the nodes — whose size is the capacity, and which launchQuery keys on — are made last: a failure
        // of either allocation leaves no wide tree and capacity 0, so the next build allocates again
        s->tlas8.reset(); s->tlas8Refs.reset();
        HIP_TRY(s->tlas8Refs.alloc(cap));
        HIP_TRY(s->tlas8.alloc(cap * 5));
        s->bytes += cap * 84;
    }
    if (int r = reserveTlasWideScratch(s)) return r;
    const uint32_t cap8 = (uint32_t)(s->tlas8.count() / 5);
    launch_tlas8_build(s->nodes, (uint32_t)s->nTlasNodes, s->tlasIdx, (uint32_t)s->nTlasIdx, s->instances, (uint32_t)s->nInst, s->tlas8, cap8, s->tlas8Refs,
                       cap8, s->tlas4Scratch, c->status, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int buildTlasWide4(tbvh_scene* s) {
    tbvh_context* c = s->ctx;
    const uint64_t cap = tlas4_cap_blocks(s->nTlasNodes, s->nInst);
    if (cap > 0x7fffffffull) {   // beyond 31-bit block offsets: the flat loop serves this TLAS; drop a 4-wide TLAS of an earlier, smaller upload
        s->tlas4.reset();
        return 0;
    }
    if (cap > s->tlas4.count()) {
        HIP_TRY(s->tlas4.alloc(cap));
        s->bytes += cap * 16;
    }
    if (int r = reserveTlasWideScratch(s)) return r;
    launch_tlas4_build(s->nodes, (uint32_t)s->nTlasNodes, s->tlasIdx, (uint32_t)s->nTlasIdx, s->instances, (uint32_t)s->nInst, s->tlas4, (uint32_t)s->tlas4.count(), s->tlas4Scratch, c->status, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int buildTlas4(tbvh_scene* s) {
    const bool any2 = (bool)s->blasDescAny;
    const bool want8 = s->blasLayout == TBVH_LAYOUT_CWBVH || s->blasMixCw2 || (any2 && (s->blasLayoutAny == TBVH_LAYOUT_CWBVH || s->blasMixCw2Any));
    const bool want4 = s->blasLayout == TBVH_LAYOUT_BVH4_GPU || (any2 && s->blasLayoutAny == TBVH_LAYOUT_BVH4_GPU);
    if (want8) if (int r = buildTlasWide8(s)) return r;   // (the two builds share the scratch area: in order on one stream)
    if (want4) if (int r = buildTlasWide4(s)) return r;
    return 0;
}

int tlasCopy(tbvh_scene* s, const void* nodes64, uint64_t nNodes, const uint32_t* idx, uint64_t nIdx, const void* inst, uint64_t nInst) {
    tbvh_context* c = s->ctx;
    // same hardening as the BLAS uploads: the TLAS kernels index instances[idx[]] and blas[blasIdx] unguarded
    if (const char* why = validate_bvh_gpu((const NodeAL*)nodes64, nNodes, nIdx)) return fail(why == kValidateNoMemory ? TBVH_E_NOMEM : TBVH_E_FORMAT, "TLAS: %s", why);
    for (uint64_t i = 0; i < nIdx; i++) if (idx[i] >= nInst) return fail(TBVH_E_FORMAT, "TLAS: primIdx[%llu] = %u is not an instance (%llu instances)", (unsigned long long)i, idx[i], (unsigned long long)nInst);
    const BLASInstanceCheck* ic = (const BLASInstanceCheck*)inst;
    for (uint64_t i = 0; i < nInst; i++) if (ic[i].blasIdx >= s->nBlas) return fail(TBVH_E_FORMAT, "instance %llu: blasIdx %u out of range (%llu BLASes)", (unsigned long long)i, ic[i].blasIdx, (unsigned long long)s->nBlas);
    HIP_TRY(s->nodes.reserve(nNodes * 4));
    HIP_TRY(s->tlasIdx.reserve(nIdx));
    HIP_TRY(s->instances.reserve(nInst * 12));
    HIP_TRY(hipMemcpyAsync(s->nodes, nodes64, nNodes * 64, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(s->tlasIdx, idx, nIdx * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(s->instances, inst, nInst * 192, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller may reuse its host arrays right away
    s->bytes = nNodes * 64 + nIdx * 4 + nInst * 192;
    s->nInst = nInst; s->nTlasNodes = nNodes; s->nTlasIdx = nIdx;
    return buildTlas4(s);
}
}  // namespace

extern "C++" {
namespace tbvh_capi {
// The BLAS descriptors of TLAS t and the class of two-level kernel that serves each kind of query, from its BLASes as they are NOW (their copies come and
// go: a tbvh_update_* drops them, queries bring them back, tbvh_set_variant switches between copy and nodes); builds the wide TLAS(es) those kernels walk.
// With every BLAS copied, BLASes of different layouts under one TLAS share one kernel class per kind of query instead of the flat three-state loop.
int reclassifyTlas(tbvh_scene* t) {
    const size_t nBlas = t->blasList.size();
    if (t->blasSpheres) {   // sphere BLASes (capi_custom.hip): one class for both kinds of query, every BLAS through its own arrays (no copies, no wide TLAS)
        std::vector<BlasDesc> desc(nBlas);
        int layout = 0;
        for (size_t i = 0; i < nBlas; i++) {
            const tbvh_scene* b = t->blasList[i];
            layout = i == 0 ? b->layout : (layout == b->layout ? layout : 0);
            desc[i] = BlasDesc{b->nodes, b->tris, b->opmap, b->opmapN, (uint32_t)b->layout};
        }
        t->blasLayout = layout; t->blasMixCw2 = false; t->blasLayoutAny = -1; t->blasMixCw2Any = false;
        if (!t->blasDesc) HIP_TRY(t->blasDesc.alloc(nBlas));
        HIP_TRY(hipStreamSynchronize(t->ctx->stream));   // (launches in flight read the old descriptors)
        HIP_TRY(hipMemcpy(t->blasDesc, desc.data(), nBlas * sizeof(BlasDesc), hipMemcpyHostToDevice));
        t->blasDescAny.reset();
        return 0;
    }
    std::vector<BlasDesc> desc[2] = {std::vector<BlasDesc>(nBlas), std::vector<BlasDesc>(nBlas)};
    int layout[2] = {0, 0};
    bool mix[2] = {false, false}, same = true;
    for (int pass = 0; pass < 3; pass++) {
        // pass 0: closest hits, BVH_GPU / BVH8_CWBVH BLASes through their 4-wide copies; pass 1 (only if pass 0 ended in the flat loop: a BLAS too small
        // for a copy next to copied ones): closest hits without the 4-wide copies; pass 2: any-hit queries
        const int any = pass == 2;
        if (pass == 1 && (layout[0] != 0 || mix[0])) continue;
        bool anyBvh4 = false;
        for (size_t i = 0; i < nBlas; i++) {
            const tbvh_scene* b = t->blasList[i];
            const tbvh_scene* v = blasView(b, any != 0, pass == 0);
            layout[any] = i == 0 ? v->layout : (layout[any] == v->layout ? layout[any] : 0);   // 0: the BLASes mix layouts (traverse_tlas.cl:50-72)
            anyBvh4 |= v->layout == TBVH_LAYOUT_BVH4_GPU;
            desc[any][i].nodes = v->nodes; desc[any][i].tris = v->tris; desc[any][i].opmap = b->opmap; desc[any][i].opmapN = b->opmapN; desc[any][i].layout = (uint32_t)v->layout;
            if (any) same &= desc[1][i].nodes == desc[0][i].nodes;
        }
        mix[any] = layout[any] == 0 && !anyBvh4;
    }
    // a class of its own for any-hit queries only where it is served by the 8-wide kernel (some BVH4_GPU BLASes with a copy and some without would
    // take the flat loop: then IsOccluded stays with Intersect's arrays)
    const bool any2 = t->anyHitSeen && !same && (layout[1] == TBVH_LAYOUT_CWBVH || mix[1]);
    t->blasLayout = layout[0]; t->blasMixCw2 = mix[0];
    t->blasLayoutAny = any2 ? layout[1] : -1; t->blasMixCw2Any = any2 && mix[1];
    if (!t->blasDesc) HIP_TRY(t->blasDesc.alloc(nBlas));
    HIP_TRY(hipStreamSynchronize(t->ctx->stream));   // (launches in flight read the old descriptors)
    HIP_TRY(hipMemcpy(t->blasDesc, desc[0].data(), nBlas * sizeof(BlasDesc), hipMemcpyHostToDevice));
    if (any2) {
        if (!t->blasDescAny) HIP_TRY(t->blasDescAny.alloc(nBlas));
        HIP_TRY(hipMemcpy(t->blasDescAny, desc[1].data(), nBlas * sizeof(BlasDesc), hipMemcpyHostToDevice));
    } else t->blasDescAny.reset();
    if (t->nodes) return buildTlas4(t);
    return 0;
}
}  // namespace tbvh_capi
}  // extern "C++"

int tbvh_upload_tlas(tbvh_context* c, const void* nodes64, uint64_t nNodes, const uint32_t* idx, uint64_t nIdx, const void* inst,
                     uint64_t nInst, tbvh_scene* const* blas, uint64_t nBlas, tbvh_scene** out) {
    if (!c || !nodes64 || !idx || !inst || !blas || !out || !nNodes || !nIdx || !nInst || !nBlas) return fail(TBVH_E_INVALID, "tbvh_upload_tlas: null/empty argument");
    for (uint64_t i = 0; i < nBlas; i++) {
        const tbvh_scene* b = blas[i];
        if (!b || b->ctx != c || b->isTlas || b->zombie) return fail(TBVH_E_INVALID, "BLAS %llu is null, freed, a TLAS, or from another context", (unsigned long long)i);
        if (b->layout != TBVH_LAYOUT_CWBVH && b->layout != TBVH_LAYOUT_BVH4_GPU && b->layout != TBVH_LAYOUT_BVH_GPU && b->layout != TBVH_LAYOUT_VOXELSET &&
            b->layout != TBVH_LAYOUT_BVH2_WALD)
            return fail(TBVH_E_INVALID, "BLAS %llu: layout %d cannot be a BLAS", (unsigned long long)i, b->layout);
        // voxel sets only all together (kernels_voxel.hip); a TLAS mixing them with triangle BLASes would need the kernels_tlas* loops to enter them
        if ((b->layout == TBVH_LAYOUT_VOXELSET) != (blas[0]->layout == TBVH_LAYOUT_VOXELSET))
            return fail(TBVH_E_INVALID, "BLAS %llu: a TLAS over voxel sets takes voxel sets only (BLAS 0 has layout %d, this one %d)", (unsigned long long)i, blas[0]->layout, b->layout);
    }
    // sphere BLASes (capi_custom.hip) alone or with triangle BLASes: the flat loop with the sphere step enters every BLAS in its own layout, no copies
    bool spheres = false;
    for (uint64_t i = 0; i < nBlas; i++) spheres |= blas[i]->layout == TBVH_LAYOUT_BVH2_WALD;
    TBVH_ENTER(c);
    for (uint64_t i = 0; i < nBlas && !spheres; i++)   // closest-hit queries enter BVH_GPU and BVH8_CWBVH BLASes through 4-wide copies (blasView), made now; the 8-wide copies any-hit queries
                                                       // enter BVH_GPU and BVH4_GPU BLASes through are made by the TLAS's first any-hit query (launchQuery)
        makeCopyOnce(blas[i], kCopyWide4);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_BVH_GPU);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    s->isTlas = true; s->nBlas = nBlas; s->blasSpheres = spheres;
    s->blasLayout = -1;   // (not classified yet)
    for (uint64_t i = 0; i < nBlas; i++) { s->blasList.push_back(blas[i]); blas[i]->usedBy.push_back(s); }
    if (int r = reclassifyTlas(s)) { tbvh_free_scene(s); return r; }
    if (int r = tlasCopy(s, nodes64, nNodes, idx, nIdx, inst, nInst)) { tbvh_free_scene(s); return r; }
    *out = s;
    return 0;
}

int tbvh_update_tlas(tbvh_scene* s, const void* nodes64, uint64_t nNodes, const uint32_t* idx, uint64_t nIdx, const void* inst, uint64_t nInst) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_update_tlas");
    if (!s || !s->isTlas || !nodes64 || !idx || !inst || !nNodes || !nIdx || !nInst) return fail(TBVH_E_INVALID, "tbvh_update_tlas: not a TLAS or null/empty argument");
    TBVH_ENTER(s->ctx);
    return tlasCopy(s, nodes64, nNodes, idx, nIdx, inst, nInst);
}

// ---- in-place re-upload of a BLAS whose blob the caller refitted / re-converted on the host ---------------------------------------------
// (BVH::Refit tiny_bvh.h:3055-3093 + X::ConvertFrom again: the reference's flow for animated geometry.)  The device allocations, the scene
// handle and the pointers the TLASes over this BLAS hold stay as they are; the library's derived copies follow.
static int updateBvhGpuImpl(const char* who, tbvh_scene* s, const void* nodes64, uint64_t nNodes, const uint32_t* primIdx, uint64_t nIdx, const tbvh_mesh* mesh) {
    TBVH_REFUSE_DOUBLE(s, who);
    TBVH_REFUSE_VOXEL(s, who);
    TBVH_REFUSE_CUSTOM(s, who);
    if (!s || s->isTlas || s->layout != TBVH_LAYOUT_BVH_GPU || !nodes64 || !primIdx || !mesh || !mesh->verts || !nNodes) return fail(TBVH_E_INVALID, "%s: not a BVH_GPU scene or null/empty argument", who);
    if (nNodes * 4 > s->capNodeBlocks || nIdx * 3 > s->capTriBlocks) return fail(TBVH_E_INVALID, "%s: the blob (%llu nodes, %llu indices) is larger than the one uploaded: free the scene and upload", who, (unsigned long long)nNodes, (unsigned long long)nIdx);
    if (const char* why = validate_bvh_gpu((const NodeAL*)nodes64, nNodes, nIdx)) return fail(why == kValidateNoMemory ? TBVH_E_NOMEM : TBVH_E_FORMAT, "%s", why);
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    const BvhGpuFill f = fillBvhGpu(s, hipSuccess, nodes64, nNodes, primIdx, nIdx, *mesh);
    if (f.e != hipSuccess) return fail(TBVH_E_HIP, "%s: %s", who, hipGetErrorString(f.e));
    if (!f.indexed && s->meshIdx) {   // re-uploaded from vertices without indices: a held index buffer would describe another mesh
        s->meshIdx.reset();
        s->bytes -= s->meshIdxTris * 12; s->meshIdxTris = 0;
    }
    s->nNodeBlocks = nNodes * 4; s->nTriBlocks = nIdx * 3;
    dropCopiesAfterUpdate(s);   // (the copies are of the old tree: they come back once the blob has settled — copy_policy.h)
    return !f.r && f.general ? checkStatus(c) : f.r;
}

int tbvh_update_bvh_gpu(tbvh_scene* s, const void* nodes64, uint64_t nNodes, const uint32_t* primIdx, uint64_t nIdx, const void* verts16, uint64_t nTris) {
    const tbvh_mesh m = flatMesh(verts16, nTris, 0);
    return updateBvhGpuImpl("tbvh_update_bvh_gpu", s, nodes64, nNodes, primIdx, nIdx, &m);
}

int tbvh_update_bvh_gpu_mesh(tbvh_scene* s, const void* nodes64, uint64_t nNodes, const uint32_t* primIdx, uint64_t nIdx, const tbvh_mesh* mesh) {
    if (s && s->layout == TBVH_LAYOUT_BVH_GPU && !s->isTlas) if (int r = checkMesh(mesh, "tbvh_update_bvh_gpu_mesh")) return r;
    return updateBvhGpuImpl("tbvh_update_bvh_gpu_mesh", s, nodes64, nNodes, primIdx, nIdx, mesh);
}

int tbvh_update_bvh4_gpu(tbvh_scene* s, const void* blocks16, uint64_t nBlocks) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_update_bvh4_gpu");
    TBVH_REFUSE_VOXEL(s, "tbvh_update_bvh4_gpu");
    TBVH_REFUSE_CUSTOM(s, "tbvh_update_bvh4_gpu");
    if (!s || s->isTlas || s->layout != TBVH_LAYOUT_BVH4_GPU || !blocks16 || nBlocks < 4) return fail(TBVH_E_INVALID, "tbvh_update_bvh4_gpu: not a BVH4_GPU scene or null/empty argument");
    if (nBlocks > s->capNodeBlocks) return fail(TBVH_E_INVALID, "tbvh_update_bvh4_gpu: the blob (%llu blocks) is larger than the one uploaded (%llu): free the scene and upload", (unsigned long long)nBlocks, (unsigned long long)s->capNodeBlocks);
    if (const char* why = validate_bvh4_gpu((const Vec4*)blocks16, nBlocks)) return fail(why == kValidateNoMemory ? TBVH_E_NOMEM : TBVH_E_FORMAT, "%s", why);
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    HIP_TRY(hipMemcpyAsync(s->nodes, blocks16, nBlocks * 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    s->nNodeBlocks = nBlocks;
    s->b4Levels.clear();   // (the node list of a device refit is rebuilt by the next tbvh_refit)
    s->refitScratch.reset();
    dropCopiesAfterUpdate(s);   // (the copy is of the old tree: it comes back once the blob has settled — copy_policy.h)
    return 0;
}

static int updateCwbvhImpl(tbvh_scene* s, const void* nodes16, uint64_t nNodeBlocks, const void* tris16, uint64_t nTriBlocks) {
    if (!s || s->isTlas || s->layout != TBVH_LAYOUT_CWBVH || !nodes16 || nNodeBlocks < 5 || (nTriBlocks && !tris16)) return fail(TBVH_E_INVALID, "tbvh_update_cwbvh: not a BVH8_CWBVH scene or null/empty argument");
    if (nNodeBlocks % 5) return fail(TBVH_E_FORMAT, "CWBVH node blocks (%llu) not a multiple of 5", (unsigned long long)nNodeBlocks);
    if (nNodeBlocks > s->capNodeBlocks || nTriBlocks > s->capTriBlocks) return fail(TBVH_E_INVALID, "tbvh_update_cwbvh: the blob (%llu + %llu blocks) is larger than the one uploaded (%llu + %llu): free the scene and upload",
                                                                                    (unsigned long long)nNodeBlocks, (unsigned long long)nTriBlocks, (unsigned long long)s->capNodeBlocks, (unsigned long long)s->capTriBlocks);
    if (const char* why = validate_cwbvh((const Vec4*)nodes16, nNodeBlocks / 5, nTriBlocks)) return fail(why == kValidateNoMemory ? TBVH_E_NOMEM : TBVH_E_FORMAT, "%s", why);
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    HIP_TRY(hipMemcpyAsync(s->nodes, nodes16, nNodeBlocks * 16, hipMemcpyHostToDevice, c->stream));
    if (nTriBlocks) HIP_TRY(hipMemcpyAsync(s->tris, tris16, nTriBlocks * 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // the caller may reuse its arrays
    const uint32_t nNodes = (uint32_t)(nNodeBlocks / 5);
    const uint64_t hash = cwbvhTopologyHash((const Vec4*)nodes16, nNodes);
    const bool sameShape = nNodes == s->nNodes && nTriBlocks == s->nTriBlocks && hash == s->topoHash;
    s->bytes -= (s->nNodeBlocks + s->nTriBlocks) * 16; s->bytes += (nNodeBlocks + nTriBlocks) * 16;
    s->nNodes = nNodes; s->nNodeBlocks = nNodeBlocks; s->nTriBlocks = nTriBlocks; s->topoHash = hash;
    s->refitScratch.reset();   // (sized and filled for the old tree)
    if (!sameShape) for (auto& kind : s->cohTuner) for (CohTuner& tu : kind) if (!tu.pinned) { tu.drop_pending(); tu = CohTuner(); }   // (its timings were taken on the old tree)
    if (sameShape) return rederiveCwbvhLayouts(s);   // boxes and vertices moved, the tree did not: the derived copies keep their numbering and are re-derived on the device
    // another tree in the same allocation: the derived copies go; they come back as at upload
    s->bytes = (nNodeBlocks + nTriBlocks) * 16 + s->opmapBytes;
    return resetCwbvhLayouts(s);
}

int tbvh_update_cwbvh(tbvh_scene* s, const void* nodes16, uint64_t nNodeBlocks, const void* tris16, uint64_t nTriBlocks) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_update_cwbvh");
    TBVH_REFUSE_VOXEL(s, "tbvh_update_cwbvh");
    TBVH_REFUSE_CUSTOM(s, "tbvh_update_cwbvh");
    if (s && !s->isTlas && ((s->copies.live() & kCopyWide4) || s->copies.pending())) {   // the 4-wide copy TLASes enter this BLAS through is of the old tree (also if the update is refused: harmless)
        TBVH_ENTER(s->ctx);
        dropCopiesAfterUpdate(s);
    }
    return updateCwbvhImpl(s, nodes16, nNodeBlocks, tris16, nTriBlocks);
}

namespace {
// BVH2 (device arrays) -> CWBVH scene.  msBefore: device time already spent on this request (builder), added to the report.
int convertDeviceImpl4(tbvh_context* c, const float4* dN2, uint64_t nNodes2, const uint32_t* dIdx, uint64_t nIdx, const MeshSrc& dV, tbvh_scene** out) {
    DevBuf<float4> blocks;
    DevBuf<uint2> itA, itB;
    DevBuf<uint32_t> cnt;
    const uint64_t capItems = nNodes2 / 2 + 2, capBlocks = capItems * 4 + nIdx * 3;
    if (capBlocks > 0xffffffffull) return fail(TBVH_E_INVALID, "BVH2 -> BVH4_GPU: stream would exceed 32-bit block indices");
    HIP_TRY(blocks.alloc(capBlocks));
    HIP_TRY(itA.alloc(capItems)); HIP_TRY(itB.alloc(capItems)); HIP_TRY(cnt.alloc(4));
    uint64_t nBlocks = 0; uint32_t levels = 0;
    HIP_TRY(run_convert_bvh4(dN2, (uint32_t)nNodes2, dIdx, nIdx, dV, blocks, capBlocks, itA, itB, cnt, c->status, c->stream, &nBlocks, &levels));
    uint32_t st = 0;
    HIP_TRY(hipMemcpy(&st, c->status, 4, hipMemcpyDeviceToHost));
    if (st & kStatusMeshIndex) { hipMemset(c->status, 0, 4); return fail(TBVH_E_FORMAT, "BVH2 -> BVH4_GPU: mesh: a vertex index is not a vertex (index >= n_verts)"); }
    if (st & 12u) {
        hipMemset(c->status, 0, 4);
        return fail(TBVH_E_FORMAT, (st & 8u) ? "BVH2 -> BVH4_GPU: a node's inline triangles exceed the 16-bit relative offset (leaves too large)"
                                             : "BVH2 -> BVH4_GPU: malformed BVH2 (child, primitive or triangle index out of range)");
    }
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_BVH4_GPU);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    hipError_t e = s->nodes.alloc(nBlocks);
    if (e == hipSuccess) e = hipMemcpyAsync(s->nodes, blocks, nBlocks * 16, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { tbvh_free_scene(s); return fail(TBVH_E_HIP, "BVH2 -> BVH4_GPU: %s", hipGetErrorString(e)); }
    s->nNodeBlocks = nBlocks; s->capNodeBlocks = nBlocks; s->bytes = nBlocks * 16;
    *out = s;
    return 0;
}

}  // namespace
extern "C++" {
namespace tbvh_capi {
int convertDeviceImpl(tbvh_context* c, int layout, const float4* dN2, uint64_t nNodes2, const uint32_t* dIdx, uint64_t nIdx, const MeshSrc& dV, tbvh_scene** out) {
    if (layout == TBVH_LAYOUT_BVH4_GPU) return convertDeviceImpl4(c, dN2, nNodes2, dIdx, nIdx, dV, out);
    DevBuf<float4> nodes, tris;
    DevBuf<uint2> itA, itB;
    DevBuf<uint32_t> cnt;
    // worst case: every BVH2 interior node becomes a wide node ((n + 1) / 2 of them in a full binary tree, + the root)
    const uint32_t capNodes = (uint32_t)(nNodes2 / 2 + 2);
    HIP_TRY(nodes.alloc((size_t)capNodes * 5)); HIP_TRY(tris.alloc(nIdx * 3));
    HIP_TRY(itA.alloc(capNodes)); HIP_TRY(itB.alloc(capNodes)); HIP_TRY(cnt.alloc(4));
    uint32_t nWide = 0, levels = 0; uint64_t nWideTris = 0;
    HIP_TRY(run_convert_cwbvh(dN2, (uint32_t)nNodes2, dIdx, nIdx, dV, nodes, capNodes, tris, nIdx, itA, itB, cnt, c->status, c->stream, &nWide, &nWideTris, &levels));
    uint32_t st = 0;
    HIP_TRY(hipMemcpy(&st, c->status, 4, hipMemcpyDeviceToHost));
    if (st & kStatusMeshIndex) { hipMemset(c->status, 0, 4); return fail(TBVH_E_FORMAT, "BVH2 -> CWBVH: mesh: a vertex index is not a vertex (index >= n_verts)"); }
    if (st & 12u) {
        hipMemset(c->status, 0, 4);
        return fail(TBVH_E_FORMAT, (st & 8u) ? "BVH2 -> CWBVH: a BVH2 leaf holds more than 3 triangles (SplitLeafs(3) first, like BVH8_CWBVH::ConvertFrom)"
                                             : "BVH2 -> CWBVH: malformed BVH2 (child, primitive or triangle index out of range)");
    }
    if (((uint64_t)nWide * 5) >> 32) return fail(TBVH_E_FORMAT, "BVH2 -> CWBVH: %u nodes are beyond the layout's 32-bit block index", nWide);   // (as tbvh_upload_cwbvh refuses them)
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_CWBVH);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    // keep exactly what was produced
    hipError_t e = s->nodes.alloc((size_t)nWide * 5);
    if (e == hipSuccess) e = s->tris.alloc((nWideTris ? nWideTris : 1) * 3);
    if (e == hipSuccess) e = hipMemcpyAsync(s->nodes, nodes, (size_t)nWide * 80, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess && nWideTris) e = hipMemcpyAsync(s->tris, tris, nWideTris * 48, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { tbvh_free_scene(s); return fail(TBVH_E_HIP, "BVH2 -> CWBVH: %s", hipGetErrorString(e)); }
    s->nNodes = nWide; s->nNodeBlocks = (uint64_t)nWide * 5; s->nTriBlocks = nWideTris * 3;
    s->capNodeBlocks = s->nNodeBlocks; s->capTriBlocks = nWideTris ? s->nTriBlocks : 3;
    s->bytes = (s->nNodeBlocks + s->nTriBlocks) * 16;
    if (int r = resetCwbvhLayouts(s, true)) { tbvh_free_scene(s); return r; }   // (level order is close to priority order: the incoherent-batch copies need no renumbering)
    *out = s;
    return 0;
}
}  // namespace tbvh_capi
}  // extern "C++"

// tail of a device conversion / build (r: its code): a scene made from an indexed mesh keeps the indices; a failure there frees it
static int keepIndicesOrFree(const char* who, int r, const MeshSrc& src, tbvh_scene** out) {
    if (r || !src.indices) return r;
    r = keepMeshIndices(*out, src);
    if (!r && hipStreamSynchronize((*out)->ctx->stream) != hipSuccess) r = fail(TBVH_E_HIP, "%s: copying the index buffer failed", who);
    if (r) { tbvh_free_scene(*out); *out = nullptr; }
    return r;
}

static int convertBvh2Impl(const char* who, tbvh_context* c, const void* nodes32, uint64_t nNodes2, const uint32_t* primIdx, uint64_t nIdx, const tbvh_mesh& mesh,
                           int onDevice, int layout, tbvh_scene** out) {
    if (layout != TBVH_LAYOUT_CWBVH && layout != TBVH_LAYOUT_BVH4_GPU) return fail(TBVH_E_INVALID, "%s: target layout %d not supported (BVH8_CWBVH and BVH4_GPU are)", who, layout);
    if (nNodes2 > 0x7fffffffull || nIdx > 0x7fffffffull) return fail(TBVH_E_INVALID, "%s: BVH2 too large for 32-bit node / triangle indices", who);
    TBVH_ENTER(c);
    DevBuf<float4> ownN2;
    DevBuf<uint32_t> ownIdx;
    DeviceMesh dm;
    const float4* dN2 = (const float4*)nodes32;
    const uint32_t* dIdx = primIdx;
    if (!onDevice) {
        HIP_TRY(ownN2.alloc(nNodes2 * 2)); HIP_TRY(ownIdx.alloc(nIdx));
        HIP_TRY(hipMemcpyAsync(ownN2, nodes32, nNodes2 * 32, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(ownIdx, primIdx, nIdx * 4, hipMemcpyHostToDevice, c->stream));
        dN2 = ownN2; dIdx = ownIdx;
    }
    if (int r = stageMesh(c, mesh, dm)) return r;
    HIP_TRY(timedBegin(c));
    int r = convertDeviceImpl(c, layout, dN2, nNodes2, dIdx, nIdx, dm.src, out);
    HIP_TRY(timedEnd(c));
    return keepIndicesOrFree(who, r, dm.src, out);
}

int tbvh_convert_bvh2_device(tbvh_context* c, const void* nodes32, uint64_t nNodes2, const uint32_t* primIdx, uint64_t nIdx, const void* verts16,
                             uint64_t nTris, int onDevice, int layout, tbvh_scene** out) {
    if (!c || !nodes32 || !primIdx || !verts16 || !out || nNodes2 == 0 || nIdx == 0 || nTris == 0) return fail(TBVH_E_INVALID, "tbvh_convert_bvh2_device: null/empty argument");
    return convertBvh2Impl("tbvh_convert_bvh2_device", c, nodes32, nNodes2, primIdx, nIdx, flatMesh(verts16, nTris, onDevice), onDevice, layout, out);
}

int tbvh_convert_bvh2_device_mesh(tbvh_context* c, const void* nodes32, uint64_t nNodes2, const uint32_t* primIdx, uint64_t nIdx, const tbvh_mesh* mesh,
                                  int onDevice, int layout, tbvh_scene** out) {
    if (!c || !nodes32 || !primIdx || !out || nNodes2 == 0 || nIdx == 0) return fail(TBVH_E_INVALID, "tbvh_convert_bvh2_device_mesh: null/empty argument");
    if (int r = checkMesh(mesh, "tbvh_convert_bvh2_device_mesh")) return r;
    return convertBvh2Impl("tbvh_convert_bvh2_device_mesh", c, nodes32, nNodes2, primIdx, nIdx, *mesh, onDevice, layout, out);
}

namespace {
// builder: 0 = LBVH (maxLeafTris applies), 1 = PLOC (one triangle per leaf; radius = search window to each side), 2 = the reference's binned-SAH
// tree (kernels_sahbuild.hip; maxLeafTris = SplitLeafs)
int buildDeviceImpl(const char* who, tbvh_context* c, const tbvh_mesh& mesh, int layout, uint32_t maxLeafTris, int builder, uint32_t radius, tbvh_scene** out) {
    const uint64_t nTris = mesh.n_tris;
    if (!c || !mesh.verts || !out || nTris == 0) return fail(TBVH_E_INVALID, "%s: null/empty argument", who);
    if (layout != TBVH_LAYOUT_CWBVH && layout != TBVH_LAYOUT_BVH4_GPU) return fail(TBVH_E_INVALID, "%s: target layout %d not supported (BVH8_CWBVH and BVH4_GPU are)", who, layout);
    if (nTris > 0x3fffffffull) return fail(TBVH_E_INVALID, "%s: too many triangles for 32-bit node indices", who);
    TBVH_ENTER(c);
    DevBuf<float4> n2;
    DevBuf<uint32_t> idx;
    DevBuf<void> scratch;
    DeviceMesh dm;
    if (int r = stageMesh(c, mesh, dm)) return r;
    size_t sortTemp = 0, scanTemp = 0;
    const size_t scratchBytes = builder == 2 ? sah_scratch_bytes((uint32_t)nTris, &sortTemp, &scanTemp)
                              : builder == 1 ? ploc_scratch_bytes((uint32_t)nTris, &sortTemp, &scanTemp) : lbvh_scratch_bytes((uint32_t)nTris, &sortTemp);
    HIP_TRY(n2.alloc(nTris * 4)); HIP_TRY(idx.alloc(nTris)); HIP_TRY(scratch.alloc(scratchBytes));
    HIP_TRY(timedBegin(c));
    if (builder == 2) {
        uint32_t nNodes = 0;
        HIP_TRY(run_sah_build(dm.src, (uint32_t)nTris, maxLeafTris, c->sahSmallSubtree, c->sahOneGroup, n2, idx, scratch, sortTemp, scanTemp, c->status, c->stream, &nNodes));
        scratch.reset();
        int r = convertDeviceImpl(c, layout, n2, nNodes, idx, nTris, dm.src, out);
        HIP_TRY(timedEnd(c));
        return keepIndicesOrFree(who, r, dm.src, out);
    }
    if (builder == 1) HIP_TRY(launch_ploc_build(dm.src, (uint32_t)nTris, radius, n2, idx, scratch, sortTemp, scanTemp, c->stream, nullptr));
    else HIP_TRY(launch_lbvh_build(dm.src, (uint32_t)nTris, maxLeafTris, n2, idx, scratch, sortTemp, c->stream));
    int r = convertDeviceImpl(c, layout, n2, nTris * 2, idx, nTris, dm.src, out);
    HIP_TRY(timedEnd(c));
    return keepIndicesOrFree(who, r, dm.src, out);
}
}  // namespace

// LBVH leaf size: 0 = the layout's default; false: more than the layout holds
static bool lbvhLeafTris(const char* who, int layout, uint32_t& maxLeafTris) {
    const uint32_t leafCap = layout == TBVH_LAYOUT_CWBVH ? 3u : 4u;
    // default: one triangle per leaf for CWBVH.  Contiguous Morton ranges make poor multi-triangle leaves: measured on the
    // Bistro stand-in, 1 / 2 / 3 triangles per leaf trace camera rays at 3629 / 3354 / 3125 and bounce rays at 2323 / 2150 /
    // 1884 MRays/s (the host SAH tree: 3300 / 2480), for 13 instead of 8 ms of build time and 22 % more memory
    if (maxLeafTris == 0) maxLeafTris = layout == TBVH_LAYOUT_CWBVH ? 1u : leafCap;
    if (maxLeafTris > leafCap) { fail(TBVH_E_INVALID, "%s: at most %u triangles per leaf for this layout", who, leafCap); return false; }
    return true;
}

int tbvh_build_device(tbvh_context* c, const void* verts16, uint64_t nTris, int onDevice, int layout, uint32_t maxLeafTris, tbvh_scene** out) {
    if (!lbvhLeafTris("tbvh_build_device", layout, maxLeafTris)) return TBVH_E_INVALID;
    return buildDeviceImpl("tbvh_build_device", c, flatMesh(verts16, nTris, onDevice), layout, maxLeafTris, 0, 0, out);
}

// SAH leaf size: 0 = what the layout's leaves hold; false: more than that
static bool sahLeafTris(const char* who, int layout, uint32_t& maxLeafTris) {
    const uint32_t leafCap = layout == TBVH_LAYOUT_CWBVH ? 3u : 4u;
    if (maxLeafTris == 0) maxLeafTris = leafCap;
    if (maxLeafTris > leafCap) { fail(TBVH_E_INVALID, "%s: at most %u triangles per leaf for this layout", who, leafCap); return false; }
    return true;
}

int tbvh_build_device_sah(tbvh_context* c, const void* verts16, uint64_t nTris, int onDevice, int layout, uint32_t maxLeafTris, tbvh_scene** out) {
    if (layout != TBVH_LAYOUT_CWBVH && layout != TBVH_LAYOUT_BVH4_GPU) return fail(TBVH_E_INVALID, "tbvh_build_device_sah: target layout %d not supported (BVH8_CWBVH and BVH4_GPU are)", layout);
    if (!sahLeafTris("tbvh_build_device_sah", layout, maxLeafTris)) return TBVH_E_INVALID;
    return buildDeviceImpl("tbvh_build_device_sah", c, flatMesh(verts16, nTris, onDevice), layout, maxLeafTris, 2, 0, out);
}

int tbvh_build_device_ploc(tbvh_context* c, const void* verts16, uint64_t nTris, int onDevice, int layout, uint32_t radius, tbvh_scene** out) {
    if (radius == 0) radius = 16;
    if (radius > 32u) return fail(TBVH_E_INVALID, "tbvh_build_device_ploc: search radius %u (1..32; 0 = the default 16)", radius);
    return buildDeviceImpl("tbvh_build_device_ploc", c, flatMesh(verts16, nTris, onDevice), layout, 1, 1, radius, out);
}

int tbvh_build_device_mesh(tbvh_context* c, const tbvh_mesh* mesh, int layout, uint32_t maxLeafTris, int builder, uint32_t radius, tbvh_scene** out) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_build_device_mesh: null argument");
    if (int r = checkMesh(mesh, "tbvh_build_device_mesh")) return r;
    if (builder == 0) { if (!lbvhLeafTris("tbvh_build_device_mesh", layout, maxLeafTris)) return TBVH_E_INVALID; }
    else if (builder == 1) {
        if (radius == 0) radius = 16;
        if (radius > 32u) return fail(TBVH_E_INVALID, "tbvh_build_device_mesh: search radius %u (1..32; 0 = the default 16)", radius);
        maxLeafTris = 1;
    } else if (builder == 2) {
        if (layout != TBVH_LAYOUT_CWBVH && layout != TBVH_LAYOUT_BVH4_GPU) return fail(TBVH_E_INVALID, "tbvh_build_device_mesh: target layout %d not supported (BVH8_CWBVH and BVH4_GPU are)", layout);
        if (!sahLeafTris("tbvh_build_device_mesh", layout, maxLeafTris)) return TBVH_E_INVALID;
    } else return fail(TBVH_E_INVALID, "tbvh_build_device_mesh: builder %d (0 = LBVH, 1 = PLOC, 2 = binned SAH)", builder);
    return buildDeviceImpl("tbvh_build_device_mesh", c, *mesh, layout, maxLeafTris, builder, radius, out);
}

namespace {
// the TLASes over BLAS b hold a snapshot of its device pointers: rewrite their entries for b
int refreshBlasDescs(tbvh_scene* b) {
    return forEachTlasOver(b, reclassifyTlas);
}
}  // namespace

int tbvh_set_opacity_micromaps(tbvh_scene* s, const uint32_t* mapData, uint32_t N, uint64_t nTris, int onDevice) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_set_opacity_micromaps");
    TBVH_REFUSE_VOXEL(s, "tbvh_set_opacity_micromaps");
    TBVH_REFUSE_CUSTOM(s, "tbvh_set_opacity_micromaps");
    if (!s || s->isTlas) return fail(TBVH_E_INVALID, "tbvh_set_opacity_micromaps: not a BLAS scene (set the maps on the BLASes before uploading their TLAS)");
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    // validate first, build the new map next, and only then swap it in: every exit leaves the scene and the TLASes over it (their BlasDesc
    // snapshots) pointing at live memory — the old maps on a failure, the new ones on success
    const bool clear = !mapData || N == 0;
    if (!clear && (N > 1024 || nTris == 0)) return fail(TBVH_E_INVALID, "tbvh_set_opacity_micromaps: N = %u, %llu triangles", N, (unsigned long long)nTris);
    DevBuf<uint32_t> fresh;
    if (!clear) {
        uint64_t words = 0;
        if (int r = allocOpacityMaps(c, N, nTris, "tbvh_set_opacity_micromaps", fresh, &words)) return r;
        hipError_t e = hipMemcpyAsync(fresh, mapData, words * 4, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(TBVH_E_HIP, "tbvh_set_opacity_micromaps: copying the maps failed: %s", hipGetErrorString(e));
    }
    return installOpacityMaps(s, std::move(fresh), clear ? 0u : N);
}

extern "C++" {
namespace tbvh_capi {
int allocOpacityMaps(tbvh_context* c, uint32_t N, uint64_t nTris, const char* who, DevBuf<uint32_t>& fresh, uint64_t* wordsOut) {
    const uint64_t wordsPerTri = ((uint64_t)N * N + 31) >> 5, words = wordsPerTri * nTris;
    // the reference's index can run one row past the map when u + v == 1 exactly (tiny_bvh.h:8518-8519): keep that read inside the allocation
    const uint64_t pad = (((uint64_t)N + 1) * (N + 1) + 63) >> 5;
    if (fresh.alloc(words + pad) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: %llu bytes of device memory", who, (unsigned long long)((words + pad) * 4)); }
    const hipError_t e = hipMemsetAsync(fresh + words, 0, pad * 4, c->stream);
    if (e != hipSuccess) return fail(TBVH_E_HIP, "%s: clearing the maps' padding failed: %s", who, hipGetErrorString(e));
    *wordsOut = words;
    return 0;
}

int installOpacityMaps(tbvh_scene* s, DevBuf<uint32_t>&& fresh, uint32_t N) {
    tbvh_context* c = s->ctx;
    HIP_TRY(hipStreamSynchronize(c->stream));   // no query may still read the old maps
    const uint64_t freshBytes = fresh.count() * 4;
    DevBuf<uint32_t> old = std::move(s->opmapOwn);
    const uint64_t oldBytes = s->opmapBytes;
    s->opmapOwn = std::move(fresh);
    s->opmap = s->opmapOwn; s->opmapN = N; s->opmapBytes = freshBytes;
    s->bytes += freshBytes; s->bytes -= oldBytes;
    shareOpacityMaps(s);
    const int r = refreshBlasDescs(s);   // the descriptors are rewritten before the old maps go
    if (r != 0) (void)old.release();   // (a failed refresh may have left a descriptor on the old maps: leak them rather than dangle)
    return r;
}
}  // namespace tbvh_capi
}  // extern "C++"

int tbvh_scene_download(tbvh_scene* s, int which, void* dst, uint64_t capBytes, uint64_t* bytesOut) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_scene_download");
    TBVH_REFUSE_VOXEL(s, "tbvh_scene_download");
    TBVH_REFUSE_CUSTOM(s, "tbvh_scene_download");
    if (!s || s->isTlas || (which != 0 && which != 1)) return fail(TBVH_E_INVALID, "tbvh_scene_download: not a BLAS scene or bad blob selector");
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    const void* src = which == 0 ? (const void*)s->nodes : (const void*)s->tris;
    const uint64_t bytes = (which == 0 ? s->nNodeBlocks : s->nTriBlocks) * 16;
    if (bytesOut) *bytesOut = src ? bytes : 0;
    if (!dst) return 0;
    if (!src) return fail(TBVH_E_INVALID, "tbvh_scene_download: this layout has no such blob");
    if (capBytes < bytes) return fail(TBVH_E_INVALID, "tbvh_scene_download: buffer too small (%llu < %llu bytes)", (unsigned long long)capBytes, (unsigned long long)bytes);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// the scene's vertex staging buffer holds `bytes` bytes of the caller's host array (asynchronous copy)
static int stageRefitVertices(tbvh_scene* s, const void* hostVerts, uint64_t bytes) {
    HIP_TRY(s->vertStage.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(s->vertStage, hostVerts, bytes, hipMemcpyHostToDevice, s->ctx->stream));
    return 0;
}

int tbvh_refit(tbvh_scene* s, const void* verts16, uint64_t nTris, int onDevice) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_refit");
    TBVH_REFUSE_VOXEL(s, "tbvh_refit");
    TBVH_REFUSE_CUSTOM(s, "tbvh_refit");
    if (!s || !verts16 || !nTris) return fail(TBVH_E_INVALID, "tbvh_refit: null/empty argument");
    if (s->isTlas) return fail(TBVH_E_INVALID, "tbvh_refit: a TLAS is rebuilt with tbvh_rebuild_tlas_device / tbvh_update_tlas");
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    if (s->layout != TBVH_LAYOUT_CWBVH && s->layout != TBVH_LAYOUT_BVH_GPU && s->layout != TBVH_LAYOUT_BVH4_GPU)
        return fail(TBVH_E_INVALID, "tbvh_refit: layout %d is not refittable", s->layout);
    const float4* dv = (const float4*)verts16;
    if (!onDevice) {
        if (int r = stageRefitVertices(s, verts16, nTris * 48)) return r;
        dv = (const float4*)s->vertStage.get();
    }
    return refitDeviceSource(s, flat_mesh(dv, nTris));
}

int tbvh_refit_mesh(tbvh_scene* s, const tbvh_mesh* mesh) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_refit_mesh");
    TBVH_REFUSE_VOXEL(s, "tbvh_refit_mesh");
    TBVH_REFUSE_CUSTOM(s, "tbvh_refit_mesh");
    if (!s) return fail(TBVH_E_INVALID, "tbvh_refit_mesh: null scene");
    if (s->isTlas) return fail(TBVH_E_INVALID, "tbvh_refit_mesh: a TLAS is rebuilt with tbvh_rebuild_tlas_device / tbvh_update_tlas");
    if (s->layout != TBVH_LAYOUT_CWBVH && s->layout != TBVH_LAYOUT_BVH_GPU && s->layout != TBVH_LAYOUT_BVH4_GPU)
        return fail(TBVH_E_INVALID, "tbvh_refit_mesh: layout %d is not refittable", s->layout);
    const bool held = mesh && !mesh->indices && s->meshIdx;   // indices == NULL on a scene made from an indexed mesh: the indices the scene holds
    if (int r = checkMesh(mesh, "tbvh_refit_mesh", held)) return r;
    if (held && mesh->n_tris != s->meshIdxTris)
        return fail(TBVH_E_INVALID, "tbvh_refit_mesh: %llu triangles, the index buffer the scene holds has %llu", (unsigned long long)mesh->n_tris, (unsigned long long)s->meshIdxTris);
    if (mesh->indices && s->meshIdx && mesh->n_tris != s->meshIdxTris)
        return fail(TBVH_E_INVALID, "tbvh_refit_mesh: new indices for %llu triangles, the scene was made from %llu", (unsigned long long)mesh->n_tris, (unsigned long long)s->meshIdxTris);
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    MeshSrc src;
    src.nTris = mesh->n_tris; src.nVerts = (uint32_t)mesh->n_verts; src.stride = mesh->stride_bytes ? mesh->stride_bytes : 16u;
    src.verts = (const float4*)mesh->verts;
    if (!mesh->on_device) {   // n_verts * stride_bytes go over the link, not n_tris * 48
        if (int r = stageRefitVertices(s, mesh->verts, meshVertexBytes(*mesh))) return r;
        src.verts = (const float4*)s->vertStage.get();
    }
    if (!mesh->indices) {
        src.indices = held ? s->meshIdx : nullptr;
        return refitDeviceSource(s, src);
    }
    // indices passed: this refit reads them where they are (host indices from a temporary device copy).  A scene that holds an index buffer takes
    // them as its new copy afterwards — device-resident ones only once the kernels have read them all without finding one out of range, so a bad
    // buffer never replaces a good one.  A scene made without indices does not start holding any: what indices == NULL means for it stays as it was.
    DevBuf<uint32_t> tmp;
    src.indices = mesh->indices;
    if (!mesh->on_device) {
        HIP_TRY(tmp.alloc(mesh->n_tris * 3));
        if (hipMemcpyAsync(tmp, mesh->indices, mesh->n_tris * 12, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(TBVH_E_HIP, "tbvh_refit_mesh: copying the indices failed");
        src.indices = tmp;
    }
    int r = refitDeviceSource(s, src);
    if (!r && mesh->on_device) r = checkStatus(c);   // (synchronizes; only the kernels have seen these indices)
    if (!r && s->meshIdx) r = keepMeshIndices(s, src);
    if (tmp) hipStreamSynchronize(c->stream);   // (the kernels and the copy above read the temporary)
    return r;
}

int tbvh_rebuild_tlas_device(tbvh_scene* s, const void* transforms, int onDevice, const float* blasBounds6, uint64_t nBlas) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_rebuild_tlas_device");
    if (!s || !s->isTlas) return fail(TBVH_E_INVALID, "tbvh_rebuild_tlas_device: not a TLAS");
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    const uint64_t n = s->nInst;
    if (n == 0 || n > 0x7fffffffull) return fail(TBVH_E_INVALID, "tbvh_rebuild_tlas_device: %llu instances", (unsigned long long)n);
    if (blasBounds6) {
        if (nBlas != s->nBlas) return fail(TBVH_E_INVALID, "tbvh_rebuild_tlas_device: %llu BLAS bounds for a TLAS over %llu BLASes", (unsigned long long)nBlas, (unsigned long long)s->nBlas);
        if (!s->blasBounds) HIP_TRY(s->blasBounds.alloc(s->nBlas * 6));
        HIP_TRY(hipMemcpyAsync(s->blasBounds, blasBounds6, s->nBlas * 24, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's array may go away
    }
    if (!s->blasBounds) return fail(TBVH_E_INVALID, "tbvh_rebuild_tlas_device: the first call needs blas_bounds6");
    // an LBVH over n leaves has 2n - 1 nodes and n index entries
    const uint64_t nNodes = 2 * n - 1;
    HIP_TRY(s->nodes.reserve(nNodes * 4));
    HIP_TRY(s->tlasIdx.reserve(n));
    if (s->buildScratchFor != n) {
        s->buildScratchFor = 0;
        HIP_TRY(s->buildScratch.alloc(tlas_build_scratch_bytes((uint32_t)n, &s->sortTempBytes)));
        s->buildScratchFor = n;
    }
    const float* xf = nullptr;
    if (transforms) {
        if (onDevice) xf = (const float*)transforms;
        else {
            HIP_TRY(s->xformStage.reserve(n * 16));   // (tbvh_update_tlas may have grown the instance array since the last rebuild)
            HIP_TRY(hipMemcpyAsync(s->xformStage, transforms, n * 64, hipMemcpyHostToDevice, c->stream));
            xf = s->xformStage;
        }
    }
    if (s->tlasBuilder == 2) {
        if (n > 0x3fffffffull) return fail(TBVH_E_INVALID, "tbvh_rebuild_tlas_device: %llu instances: the SAH builder takes at most 2^30 - 1", (unsigned long long)n);
        if (s->tlasSahFor != n) {
            s->tlasSahFor = 0;
            HIP_TRY(s->tlasSah.alloc(sah_scratch_bytes((uint32_t)n, &s->tlasSahSort, &s->tlasSahScan)));
            HIP_TRY(s->tlasWald.alloc(n * 4));
            s->tlasSahFor = n;
        }
        // the existing instance update, the reference's BVH::Build( BLASInstance*, n ) over the updated records, BVH_GPU::ConvertFrom: all on the stream
        HIP_TRY(timedBegin(c));
        HIP_TRY(launch_tlas_instance_update(s->instances, xf, s->blasBounds, (uint32_t)n, (uint32_t)s->nBlas, s->buildScratch, s->sortTempBytes, c->stream));
        uint32_t nWald = 0;
        HIP_TRY(run_sah_build(SahSrc(sah_boxes_instances(s->instances.get())), (uint32_t)n, 0, c->sahSmallSubtree, c->sahOneGroup, s->tlasWald, s->tlasIdx, s->tlasSah,
                              s->tlasSahSort, s->tlasSahScan, c->status, c->stream, &nWald));
        HIP_TRY(run_al_encode(s->tlasWald, nWald, (uint32_t)n, s->tlasSah, s->tlasSahSort, s->tlasSahScan, s->nodes, c->stream));
        s->nTlasNodes = nWald - 1; s->nTlasIdx = n;
        s->bytes = s->nTlasNodes * 64 + n * 4 + n * 192 + s->tlasSah.count() + s->tlasWald.count() * 16;
        if (int r = buildTlas4(s)) return r;
        HIP_TRY(timedEnd(c));
        return 0;
    }
    HIP_TRY(timedBegin(c));
    HIP_TRY(launch_tlas_rebuild(s->nodes, s->tlasIdx, s->instances, xf, s->blasBounds, (uint32_t)n, (uint32_t)s->nBlas, s->buildScratch, s->sortTempBytes, c->stream));
    s->bytes = nNodes * 64 + n * 4 + n * 192;
    s->nTlasNodes = nNodes; s->nTlasIdx = n;
    if (int r = buildTlas4(s)) return r;
    HIP_TRY(timedEnd(c));
    return 0;
}

int tbvh_tlas_set_builder(tbvh_scene* s, int builder) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_tlas_set_builder");
    if (!s || !s->isTlas) return fail(TBVH_E_INVALID, "tbvh_tlas_set_builder: not a TLAS");
    if (builder != 0 && builder != 2) return fail(TBVH_E_INVALID, "tbvh_tlas_set_builder: builder %d (0 = LBVH, 2 = the reference's SAH tree)", builder);
    TBVH_LOCK(s->ctx);
    s->tlasBuilder = builder;
    return 0;
}

int tbvh_tlas_download(tbvh_scene* s, void* nodes64, uint64_t capNodes, uint32_t* idx, uint64_t capIdx, void* instances192, uint64_t capInst,
                       uint64_t* nNodesOut) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_tlas_download");
    if (!s || !s->isTlas) return fail(TBVH_E_INVALID, "tbvh_tlas_download: not a TLAS");
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t n = s->nInst, nNodes = s->nTlasNodes;
    if (nNodesOut) *nNodesOut = nNodes;
    if (nodes64) { if (capNodes < nNodes) return fail(TBVH_E_INVALID, "tbvh_tlas_download: node buffer too small"); HIP_TRY(hipMemcpy(nodes64, s->nodes, nNodes * 64, hipMemcpyDeviceToHost)); }
    if (idx) { if (capIdx < n) return fail(TBVH_E_INVALID, "tbvh_tlas_download: index buffer too small"); HIP_TRY(hipMemcpy(idx, s->tlasIdx, n * 4, hipMemcpyDeviceToHost)); }
    if (instances192) { if (capInst < n) return fail(TBVH_E_INVALID, "tbvh_tlas_download: instance buffer too small"); HIP_TRY(hipMemcpy(instances192, s->instances, n * 192, hipMemcpyDeviceToHost)); }
    return 0;
}

void tbvh_free_scene(tbvh_scene* s) {
    if (!s) return;
    tbvh_context* c = s->ctx;
    TBVH_LOCK(c);
    (void)tbvh_capi::setDevice(c);   // (joins the launch lanes)
    hipStreamSynchronize(c->stream);
    if (!s->isTlas && !s->usedBy.empty()) { s->zombie = true; return; }   // a TLAS still points at this BLAS's memory: freed with the last such TLAS
    freeCopy(s, kCopyWide8);
    freeCopy(s, kCopyWide4);
    if (s->isTlas) {
        std::vector<tbvh_scene*> mine;
        mine.swap(s->blasList);
        for (tbvh_scene* b : mine) {
            for (size_t i = 0; i < b->usedBy.size(); i++) if (b->usedBy[i] == s) { b->usedBy.erase(b->usedBy.begin() + i); break; }
            if (b->zombie && b->usedBy.empty()) { b->zombie = false; tbvh_free_scene(b); }
        }
    }
    for (auto& kind : s->cohTuner) for (CohTuner& tu : kind) tu.drop_pending();
    for (size_t i = 0; i < c->scenes.size(); i++)
        if (c->scenes[i] == s) { c->scenes.erase(c->scenes.begin() + i); break; }
    delete s;   // (its device buffers go here: the device is current, the stream idle)
}
int tbvh_scene_layout(const tbvh_scene* s) { return s ? s->layout : TBVH_E_INVALID; }
uint64_t tbvh_scene_device_bytes(const tbvh_scene* s) { return s ? s->bytes : 0; }

int tbvh_debug_coherent_schedule(tbvh_scene* s, int anyhit, uint32_t out[4]) {
    if (!s || !out) return fail(TBVH_E_INVALID, "tbvh_debug_coherent_schedule: null argument");
    TBVH_LOCK(s->ctx);
    s = tunedScene(s);
    const CohTuner& t = s->cohTuner[anyhit ? 1 : 0][s->cohLastClass[anyhit ? 1 : 0]];   // (kept per batch-size class; this is the class of the most recent such launch)
    out[0] = s->ctx->cohTunerMode ? (uint32_t)s->ctx->cohTunerMode : (uint32_t)t.decided;
    out[1] = t.n[0]; out[2] = t.n[1];
    out[3] = (t.n[0] && t.n[1]) ? (uint32_t)(1000.f * t.best[1] / t.best[0]) : 0u;
    return 0;
}

// ---- the coherent-batch schedule as something a caller can read, keep and give back -------------------------------------------------------
int tbvh_scene_get_schedule_hint(tbvh_scene* s, tbvh_schedule_hint* out) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_scene_get_schedule_hint");
    TBVH_REFUSE_VOXEL(s, "tbvh_scene_get_schedule_hint");
    TBVH_REFUSE_CUSTOM(s, "tbvh_scene_get_schedule_hint");
    if (!s || !out) return fail(TBVH_E_INVALID, "tbvh_scene_get_schedule_hint: null argument");
    TBVH_LOCK(s->ctx);
    std::memset(out, 0, sizeof *out);
    s = tunedScene(s);   // (a BVH_GPU / BVH4_GPU scene: its queries run on the 8-wide copy, whose tuner decides)
    for (int k = 0; k < 3; k++) {
        out->closest_hit[k] = (uint8_t)(s->ctx->cohTunerMode ? s->ctx->cohTunerMode : s->cohTuner[0][k].decided);
        out->any_hit[k] = (uint8_t)(s->ctx->cohTunerMode ? s->ctx->cohTunerMode : s->cohTuner[1][k].decided);
    }
    // reserved[0 / 1]: the class of 768 k .. 1.5 M-ray batches on a scene under 48 MB (closest-hit / any-hit)
    out->reserved[0] = (uint8_t)(s->ctx->cohTunerMode ? s->ctx->cohTunerMode : s->cohTuner[0][3].decided);
    out->reserved[1] = (uint8_t)(s->ctx->cohTunerMode ? s->ctx->cohTunerMode : s->cohTuner[1][3].decided);
    return 0;
}

int tbvh_scene_set_schedule_hint(tbvh_scene* s, const tbvh_schedule_hint* hint) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_scene_set_schedule_hint");
    TBVH_REFUSE_VOXEL(s, "tbvh_scene_set_schedule_hint");
    TBVH_REFUSE_CUSTOM(s, "tbvh_scene_set_schedule_hint");
    if (!s || !hint) return fail(TBVH_E_INVALID, "tbvh_scene_set_schedule_hint: null argument");
    for (int k = 0; k < 3; k++) if (hint->closest_hit[k] > 3 || hint->any_hit[k] > 3) return fail(TBVH_E_INVALID, "tbvh_scene_set_schedule_hint: entries are 0 (measure), 1 (deferred + gated), 2 (strict) or 3 (one traversal per wave)");
    if (hint->reserved[0] > 3 || hint->reserved[1] > 3) return fail(TBVH_E_INVALID, "tbvh_scene_set_schedule_hint: entries are 0 (measure), 1 (deferred + gated), 2 (strict) or 3 (one traversal per wave)");
    TBVH_LOCK(s->ctx);
    s = tunedScene(s);
    for (int a = 0; a < 2; a++) for (int k = 0; k < 4; k++) {
        const uint8_t v = k == 3 ? hint->reserved[a] : a ? hint->any_hit[k] : hint->closest_hit[k];
        CohTuner& tu = s->cohTuner[a][k];
        tu.drop_pending();
        tu = CohTuner();          // (0: back to measuring, from scratch)
        if (v) { tu.decided = v; tu.pinned = true; }
    }
    return 0;
}

int tbvh_set_variant(tbvh_scene* s, int v) {
    if (!s) return fail(TBVH_E_INVALID, "null scene");
    TBVH_LOCK(s->ctx);
    // only the BVH8_CWBVH kernel keeps diagnostic variants (kernels_cwbvh.hip: forced schedules, instrumented kernels)
    // ... and BVH_GPU / BVH4_GPU scenes one: 1 = trace the nodes as uploaded (k_bvh2 / k_bvh4) even when the scene has an 8-wide copy (tests, A/B)
    const bool ok = v == 0 || (!s->isTlas && s->layout == TBVH_LAYOUT_CWBVH && cwbvh_variant_valid(v)) || (!s->isTlas && (s->layout == TBVH_LAYOUT_BVH_GPU || s->layout == TBVH_LAYOUT_BVH4_GPU) && v == 1);
    if (!ok) return fail(TBVH_E_INVALID, "unknown variant %d for layout %d", v, s->layout);
    const bool viewChanges = !s->isTlas && s->copies.live() && (s->variant == 0) != (v == 0);
    s->variant = v;
    if (viewChanges) return refreshBlasDescs(s);   // (the TLASes over this BLAS enter it through the copy, or through its own nodes)
    return 0;
}
}  // extern "C"
