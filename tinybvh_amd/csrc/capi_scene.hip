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

// ---- what a scene costs on the device ------------------------------------------------------------------------------------------------------
// A function of what the scene holds now, never of the route to it; nothing keeps a running total beside the buffers.  The rule:
//   * arrays the CALLER uploaded count at what they hold now (nNodeBlocks, nTriBlocks, nTlasNodes ...): an update with a smaller blob lowers the number,
//     whatever the allocation still has room for;
//   * buffers the LIBRARY made for itself count at their allocation (DevBuf::count()).
// The terms, one line each, with the word of tbvh_debug_scene_bytes they go to (words 0 to 6 are the number; 7 is held and NOT counted):
//   [0] the arrays as uploaded / converted / built: triangle layouts and the fp32 TLAS by their live counts, an fp64 BLAS by its node and record counts; a
//       sphere BLAS and a voxel set by their allocations (a device-built sphere tree lives in arrays the library sized for 2 n nodes)
//   [1] a BVH8_CWBVH scene's re-layouts (CwbvhLayouts): padded nodes, hybrid nodes, 64-byte triangle records
//   [2] the wide copies, each asked for ITS bytes now: a copy that grows or goes is right by construction
//   [3] opacity maps and a watertight scene's vertex copy (tbvh_set_triangle_test), on the scene that owns them (a copy shares its owner's pointer and holds none)
//   [4] the index buffer a scene made from an indexed mesh holds
//   [5] an fp32 TLAS's wide trees, the 8-wide tree's references and the SAH builder's Wald nodes; an fp64 TLAS's one allocation (capi_double.hip: tlasLayout( its
//       capacities ).total, which is what `nodes` was allocated with)
//   [6] counted scratch and staging: the SAH TLAS builder's scratch, a sphere BLAS's primIdx, an edited voxel set's work area, winner words and staged records,
//       and ON SPHERE AND fp64 SCENES ONLY buildScratch, refitScratch, vertStage
//   [7] everything else a scene holds: buildScratch, refitScratch and vertStage of every other kind of scene, idxStage, the hybrid copy's numbering (cw.perm), a
//       TLAS's shared wide-build scratch, BLAS bounds, staged transforms and descriptor tables
//       (the eight words do NOT claim to sum to the scene's allocations: the room an uploaded array keeps beyond what it holds now is in none of them)
// KNOWN INCONSISTENCY, kept as it was: a triangle scene's refit scratch (144 bytes per node: more than the tree) and staging are not counted, a sphere or fp64
// scene's are.  Counting them would move blobBytes of refitted BVH_GPU / BVH4_GPU scenes across launch_plan.h's 48 MB and 384 MB lines; that wants numbers.
SceneBytes sceneBytesByWord(const tbvh_scene* s) {
    SceneBytes b{};
    uint64_t* w = b.word;
    const TlasState& t = s->tlas;
    const bool dbl = s->layout == TBVH_LAYOUT_BVH_DOUBLE, sphere = s->layout == TBVH_LAYOUT_BVH2_WALD, voxel = s->layout == TBVH_LAYOUT_VOXELSET;
    const bool tlas32 = s->isTlas && !dbl, tlas64 = s->isTlas && dbl, blas64 = !s->isTlas && dbl;
    const bool triangles = !s->isTlas && !dbl && !sphere && !voxel;   // BVH_GPU, BVH4_GPU, BVH8_CWBVH
    if (triangles) w[0] += (s->nNodeBlocks + s->nTriBlocks) * 16;
    if (tlas32) w[0] += t.nTlasNodes * 64 + t.nTlasIdx * 4 + t.nInst * 192;
    if (blas64 && !s->dblSpheres) w[0] += (uint64_t)s->nNodes * sizeof(NodeDbl) + s->dblRecs * sizeof(TriDbl);
    if (blas64 && s->dblSpheres) w[0] += (s->nodes.count() + s->tris.count()) * 16;   // (as an fp32 sphere BLAS: what it holds at its allocation)
    if (sphere || voxel) w[0] += (s->nodes.count() + s->tris.count()) * 16;
    w[1] += (s->cw.padded.count() + s->cw.hybrid.count() + s->cw.trisPadded.count()) * 16;
    if (s->copies.copy8) w[2] += sceneBytes(s->copies.copy8);
    if (s->copies.copy4) w[2] += sceneBytes(s->copies.copy4);
    w[3] += s->opmapOwn.count() * 4 + s->wtVertsOwn.count() * 16;   // (and a watertight scene's vertices, likewise on the scene that owns them)
    w[4] += s->meshIdx.count() * 4;
    if (tlas32) w[5] += (t.tlas4.count() + t.tlas8.count() + t.tlasWald.count()) * 16 + t.tlas8Refs.count() * 4;
    if (tlas64) w[5] += s->nodes.count() * 16;
    w[6] += t.tlasSah.count() + s->sphIdx.count() * 4 + (s->voxWork.count() + s->voxWinner.count() + s->voxStage.count()) * 4;
    w[sphere || dbl ? 6 : 7] += s->buildScratch.count() + s->refitScratch.count() + s->vertStage.count();
    w[7] += (s->idxStage.count() + s->cw.perm.count()) * 4;
    w[7] += t.tlas4Scratch.count() + (t.blasBounds.count() + t.xformStage.count()) * 4 + (t.blasDesc.count() + t.blasDescAny.count()) * sizeof(BlasDesc);
    return b;
}

uint64_t sceneBytes(const tbvh_scene* s) {
    const SceneBytes b = sceneBytesByWord(s);
    uint64_t sum = 0;
    for (int k = 0; k < 7; k++) sum += b.word[k];
    return sum;
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
        if (int r = refreshWatertightVerts(s, src)) return r;   // a watertight scene tests the new vertices
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
    if (int r = refreshWatertightVerts(s, src)) return r;   // a watertight scene tests the new vertices
    return refitCopies(s, src);                      // the 8-wide and the 4-wide copy follow
}
}  // namespace tbvh_capi

extern "C" {

// ---- uploads ---------------------------------------------------------------------------

// What a BVH_GPU upload and an in-place update share (skipped when e comes in as an error): the blob's nodes go into s->nodes, its primIdx names triangles,
// whose vertices the gather finds through the mesh (flat: 3 float4 per triangle) and writes to s->tris, an indexed mesh leaves its indices with the scene
// (sceneBytes counts them); synchronous.  e: the first HIP error — the caller words it and cleans up —, r: keepMeshIndices' code; general: the gather
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
    s->nNodeBlocks = nBlocks; s->capNodeBlocks = nBlocks;
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
    if (int r = resetCwbvhLayouts(s)) { tbvh_free_scene(s); return r; }
    *out = s;
    return 0;
}

namespace {
// the 8-wide TLAS in the BVH8_CWBVH node format, from the BVH_GPU nodes on the device; asynchronous on the context's stream
int buildTlasWide8(tbvh_scene* s) {
    tbvh_context* c = s->ctx;
    TlasState& t = s->tlas;
    const uint64_t cap = tlas8_cap_nodes(t.nTlasNodes, t.nInst);
    if (cap * 5 > t.tlas8.count()) {
        // both go before either is made again, and the nodes — whose size is the capacity — are made last: a failure of either allocation leaves no wide
        // tree and capacity 0, so the next build allocates again
        t.tlas8.reset(); t.tlas8Refs.reset();
        HIP_TRY(t.tlas8Refs.alloc(cap));
        HIP_TRY(t.tlas8.alloc(cap * 5));
    }
    HIP_TRY(t.tlas4Scratch.reserve(tlas_wide_scratch_bytes(t.nTlasNodes, t.nInst)));   // (the scratch area the two wide builds share)
    const uint32_t cap8 = (uint32_t)(t.tlas8.count() / 5);
    launch_tlas8_build(s->nodes, (uint32_t)t.nTlasNodes, t.tlasIdx, (uint32_t)t.nTlasIdx, t.instances, (uint32_t)t.nInst, t.tlas8, cap8, t.tlas8Refs, cap8, t.tlas4Scratch,
                       c->status, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ... and the 4-wide one in the BVH4_GPU node format
int buildTlasWide4(tbvh_scene* s) {
    tbvh_context* c = s->ctx;
    TlasState& t = s->tlas;
    const uint64_t cap = tlas4_cap_blocks(t.nTlasNodes, t.nInst);
    if (cap > t.tlas4.count()) HIP_TRY(t.tlas4.alloc(cap));
    HIP_TRY(t.tlas4Scratch.reserve(tlas_wide_scratch_bytes(t.nTlasNodes, t.nInst)));
    launch_tlas4_build(s->nodes, (uint32_t)t.nTlasNodes, t.tlasIdx, (uint32_t)t.nTlasIdx, t.instances, (uint32_t)t.nInst, t.tlas4, (uint32_t)t.tlas4.count(), t.tlas4Scratch, c->status,
                       c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The TLAS's nodes are new (upload, update, device rebuild) or its plan is (reclassifyTlas): which wide trees fit is stated again for the TLAS's size as it
// is now, and the trees the plan wants are built from the BVH_GPU nodes on the device.  A wanted tree beyond its node format's index range is not built — the
// plan has sent those queries to the flat loop — and one left from an earlier, smaller TLAS goes, so that it is neither kept nor counted.  A tree that cannot
// be allocated is an error of the call; the plan then says "does not fit", so that no later launch walks a tree that is not there.
int buildWideTlas(tbvh_scene* s) {
    TlasState& t = s->tlas;
    const uint64_t cap8 = tlas8_cap_nodes(t.nTlasNodes, t.nInst), cap4 = tlas4_cap_blocks(t.nTlasNodes, t.nInst);
    planTlasFit(t.plan, (bool)s->nodes, cap8, cap4);
    int r = 0;
    if (t.plan.want8 && !t.plan.fits8) { t.tlas8.reset(); t.tlas8Refs.reset(); }
    if (t.plan.want4 && !t.plan.fits4) t.tlas4.reset();
    if (t.plan.fits8 && (r = buildTlasWide8(s)) != 0) planTlasFit(t.plan, true, ~0ull, cap4);   // (the two builds share the scratch area: in order on one stream)
    if (!r && t.plan.fits4 && (r = buildTlasWide4(s)) != 0) planTlasFit(t.plan, true, cap8, ~0ull);
    return r;
}

int tlasCopy(tbvh_scene* s, const void* nodes64, uint64_t nNodes, const uint32_t* idx, uint64_t nIdx, const void* inst, uint64_t nInst) {
    tbvh_context* c = s->ctx;
    TlasState& t = s->tlas;
    // same hardening as the BLAS uploads: the TLAS kernels index instances[idx[]] and blas[blasIdx] unguarded
    if (const char* why = validate_bvh_gpu((const NodeAL*)nodes64, nNodes, nIdx)) return fail(why == kValidateNoMemory ? TBVH_E_NOMEM : TBVH_E_FORMAT, "TLAS: %s", why);
    for (uint64_t i = 0; i < nIdx; i++) if (idx[i] >= nInst) return fail(TBVH_E_FORMAT, "TLAS: primIdx[%llu] = %u is not an instance (%llu instances)", (unsigned long long)i, idx[i], (unsigned long long)nInst);
    const BLASInstanceCheck* ic = (const BLASInstanceCheck*)inst;
    for (uint64_t i = 0; i < nInst; i++) if (ic[i].blasIdx >= t.nBlas) return fail(TBVH_E_FORMAT, "instance %llu: blasIdx %u out of range (%llu BLASes)", (unsigned long long)i, ic[i].blasIdx, (unsigned long long)t.nBlas);
    HIP_TRY(s->nodes.reserve(nNodes * 4));
    HIP_TRY(t.tlasIdx.reserve(nIdx));
    HIP_TRY(t.instances.reserve(nInst * 12));
    HIP_TRY(hipMemcpyAsync(s->nodes, nodes64, nNodes * 64, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(t.tlasIdx, idx, nIdx * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(t.instances, inst, nInst * 192, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller may reuse its host arrays right away
    t.nInst = nInst; t.nTlasNodes = nNodes; t.nTlasIdx = nIdx;
    return buildWideTlas(s);
}
}  // namespace

extern "C++" {
namespace tbvh_capi {
// the facts of TLAS s as they are now; `blas` holds the per-BLAS part
TlasFacts tlasFactsNow(const tbvh_scene* s, std::vector<TlasBlasFacts>& blas) {
    const TlasState& t = s->tlas;
    blas.resize(t.blasList.size());
    for (size_t i = 0; i < blas.size(); i++) blas[i] = tlasBlasFacts(t.blasList[i]);
    TlasFacts f;
    f.blas = blas.data(); f.nBlas = (uint32_t)blas.size(); f.anyHitSeen = t.anyHitSeen; f.hasNodes = (bool)s->nodes;
    f.cap8 = tlas8_cap_nodes(t.nTlasNodes, t.nInst); f.cap4 = tlas4_cap_blocks(t.nTlasNodes, t.nInst);
    return f;
}

// The plan of TLAS s (tlas_plan.h) from its BLASes as they are NOW (their copies come and go: a tbvh_update_* drops them, queries bring them back,
// tbvh_set_variant switches between copy and nodes), the one or two descriptor tables of the views it chose, the wide trees it wants.  With every BLAS
// copied, BLASes of different layouts under one TLAS share one kernel class per kind of query instead of the flat three-state loop.
int reclassifyTlas(tbvh_scene* s) {
    TlasState& t = s->tlas;
    // a watertight BVH_GPU / BVH4_GPU BLAS is entered through its 8-wide copy and nothing else: if an update dropped it, it comes back now
    for (tbvh_scene* b : t.blasList) if (b->triTest && !b->copies.copy8) if (int r = ensureWatertightCopy(b)) return r;
    std::vector<TlasBlasFacts> blas;
    const TlasFacts f = tlasFactsNow(s, blas);
    const size_t nBlas = blas.size();
    for (auto& v : t.view) v.resize(nBlas);
    TlasView* const view[2] = {t.view[0].data(), t.view[1].data()};
    t.plan = planTlas(f, view);
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));   // (launches in flight read the old descriptors)
    if (t.plan.watertight) {   // one table of BlasDescWt (kernels.h): the views' arrays and each BLAS's vertices
        for (size_t i = 0; i < nBlas; i++)
            if (!t.blasList[i]->triTest || !t.blasList[i]->wtVerts) return fail(TBVH_E_INVALID, "TLAS: BLAS %llu is not in watertight mode while others are (all or none)", (unsigned long long)i);
        std::vector<BlasDescWt> dw(nBlas);
        for (size_t i = 0; i < nBlas; i++) {
            const tbvh_scene* b = t.blasList[i];
            const tbvh_scene* v = blasView(b, t.view[0][i]);
            if (v->layout != TBVH_LAYOUT_CWBVH) return fail(TBVH_E_INVALID, "TLAS: watertight BLAS %llu has no 8-wide form to be entered through", (unsigned long long)i);
            dw[i] = BlasDescWt{BlasDesc{v->nodes, v->tris, b->opmap, b->opmapN, (uint32_t)v->layout}, b->wtVerts, b->wtTris, {0, 0}};
        }
        if (t.blasDesc.count() < nBlas * 2) { t.blasDesc.reset(); HIP_TRY(t.blasDesc.alloc(nBlas * 2)); }
        HIP_TRY(hipMemcpy(t.blasDesc, dw.data(), nBlas * sizeof(BlasDescWt), hipMemcpyHostToDevice));
        t.blasDescAny.reset();
        if (s->nodes) {
            if (int r = buildWideTlas(s)) return r;
            if (t.plan.kind[0].family != TlasFamily::kTlas8 || t.plan.kind[1].family != TlasFamily::kTlas8)
                return fail(TBVH_E_INVALID, "TLAS over watertight BLASes: the 8-wide TLAS tree does not fit, and no other two-level kernel has a watertight form");
        }
        return 0;
    }
    std::vector<BlasDesc> desc(nBlas);
    for (int kind = 0; kind < (t.plan.anyOwn ? 2 : 1); kind++) {
        for (size_t i = 0; i < nBlas; i++) {
            const tbvh_scene* b = t.blasList[i];
            const tbvh_scene* v = blasView(b, t.view[kind][i]);
            desc[i] = BlasDesc{v->nodes, v->tris, b->opmap, b->opmapN, (uint32_t)v->layout};
        }
        DevBuf<BlasDesc>& table = kind ? t.blasDescAny : t.blasDesc;
        if (!table) HIP_TRY(table.alloc(nBlas));
        HIP_TRY(hipMemcpy(table, desc.data(), nBlas * sizeof(BlasDesc), hipMemcpyHostToDevice));
    }
    if (!t.plan.anyOwn) t.blasDescAny.reset();
    if (s->nodes) return buildWideTlas(s);
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
        // a TLAS has no triangle test of its own: it reads the mode off its BLASes, which must agree — one kernel serves all of them
        bool anyWt = false;
        for (uint64_t k = 0; k < nBlas; k++) anyWt |= blas[k] && blas[k]->triTest != 0;
        if (anyWt && (b->layout == TBVH_LAYOUT_VOXELSET || b->layout == TBVH_LAYOUT_BVH2_WALD))
            return fail(TBVH_E_INVALID, "BLAS %llu is a %s next to watertight triangle BLASes (tbvh_set_triangle_test): the watertight two-level kernel enters triangle BLASes only",
                        (unsigned long long)i, b->layout == TBVH_LAYOUT_VOXELSET ? "voxel set" : "sphere BLAS");
        if ((b->triTest != 0) != (blas[0]->triTest != 0))
            return fail(TBVH_E_INVALID, "BLAS %llu is %s watertight mode (tbvh_set_triangle_test) and BLAS 0 is %s: a TLAS takes BLASes that are all watertight or all not, "
                                        "because one two-level kernel, with one triangle test, traces all of them", (unsigned long long)i, b->triTest ? "in" : "not in", blas[0]->triTest ? "in" : "not in");
        // voxel sets only all together (kernels_voxel.hip); a TLAS mixing them with triangle BLASes would need the kernels_tlas* loops to enter them
        if ((b->layout == TBVH_LAYOUT_VOXELSET) != (blas[0]->layout == TBVH_LAYOUT_VOXELSET))
            return fail(TBVH_E_INVALID, "BLAS %llu: a TLAS over voxel sets takes voxel sets only (BLAS 0 has layout %d, this one %d)", (unsigned long long)i, blas[0]->layout, b->layout);
    }
    // sphere BLASes (capi_custom.hip) alone or with triangle BLASes: the flat loop with the sphere step enters every BLAS in its own layout, no copies
    bool spheres = false;
    for (uint64_t i = 0; i < nBlas; i++) spheres |= blas[i]->layout == TBVH_LAYOUT_BVH2_WALD;
    TBVH_ENTER(c);
    if (blas[0]->triTest) { for (uint64_t i = 0; i < nBlas; i++) if (int r = ensureWatertightCopy(blas[i])) return r; }
    else for (uint64_t i = 0; i < nBlas && !spheres; i++)   // closest-hit queries enter BVH_GPU and BVH8_CWBVH BLASes through 4-wide copies (blasView), made now; the 8-wide copies any-hit queries
                                                       // enter BVH_GPU and BVH4_GPU BLASes through are made by the TLAS's first any-hit query (launchQuery)
        makeCopyOnce(blas[i], kCopyWide4);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_BVH_GPU);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    s->isTlas = true; s->tlas.nBlas = nBlas; s->tlas.blasSpheres = spheres;
    for (uint64_t i = 0; i < nBlas; i++) { s->tlas.blasList.push_back(blas[i]); blas[i]->usedBy.push_back(s); }
    if (int r = reclassifyTlas(s)) { tbvh_free_scene(s); return r; }
    if (int r = tlasCopy(s, nodes64, nNodes, idx, nIdx, inst, nInst)) { tbvh_free_scene(s); return r; }
    if (s->tlas.plan.watertight && (s->tlas.plan.kind[0].family != TlasFamily::kTlas8 || s->tlas.plan.kind[1].family != TlasFamily::kTlas8)) {
        tbvh_free_scene(s);   // (a missing kernel is an error of the upload, never another kernel at the first query)
        return fail(TBVH_E_INVALID, "TLAS over watertight BLASes: the 8-wide TLAS tree does not fit, and no other two-level kernel has a watertight form");
    }
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
        s->meshIdx.reset(); s->meshIdxTris = 0;
    }
    s->nNodeBlocks = nNodes * 4; s->nTriBlocks = nIdx * 3;
    dropCopiesAfterUpdate(s);   // (the copies are of the old tree: they come back once the blob has settled — copy_policy.h)
    if (s->triTest && !f.r) {   // a watertight scene tests the vertices this blob was made from
        DeviceMesh dm;
        if (int r = stageMesh(c, *mesh, dm)) return r;
        if (int r = refreshWatertightVerts(s, dm.src)) return r;
        HIP_TRY(hipStreamSynchronize(c->stream));   // (the staged copy goes with this call)
    }
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
    s->nNodes = nNodes; s->nNodeBlocks = nNodeBlocks; s->nTriBlocks = nTriBlocks; s->topoHash = hash;
    s->refitScratch.reset();   // (sized and filled for the old tree)
    if (!sameShape) for (auto& kind : s->cohTuner) for (CohTuner& tu : kind) if (!tu.pinned) { tu.drop_pending(); tu = CohTuner(); }   // (its timings were taken on the old tree)
    if (sameShape) return rederiveCwbvhLayouts(s);   // boxes and vertices moved, the tree did not: the derived copies keep their numbering and are re-derived on the device
    // another tree in the same allocation: the derived copies go; they come back as at upload
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
    s->nNodeBlocks = nBlocks; s->capNodeBlocks = nBlocks;
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
    DevBuf<uint32_t> old = std::move(s->opmapOwn);
    s->opmapOwn = std::move(fresh);
    s->opmap = s->opmapOwn; s->opmapN = N;
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
    const uint64_t n = s->tlas.nInst;
    if (n == 0 || n > 0x7fffffffull) return fail(TBVH_E_INVALID, "tbvh_rebuild_tlas_device: %llu instances", (unsigned long long)n);
    if (blasBounds6) {
        if (nBlas != s->tlas.nBlas) return fail(TBVH_E_INVALID, "tbvh_rebuild_tlas_device: %llu BLAS bounds for a TLAS over %llu BLASes", (unsigned long long)nBlas, (unsigned long long)s->tlas.nBlas);
        if (!s->tlas.blasBounds) HIP_TRY(s->tlas.blasBounds.alloc(s->tlas.nBlas * 6));
        HIP_TRY(hipMemcpyAsync(s->tlas.blasBounds, blasBounds6, s->tlas.nBlas * 24, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's array may go away
    }
    if (!s->tlas.blasBounds) return fail(TBVH_E_INVALID, "tbvh_rebuild_tlas_device: the first call needs blas_bounds6");
    // an LBVH over n leaves has 2n - 1 nodes and n index entries
    const uint64_t nNodes = 2 * n - 1;
    HIP_TRY(s->nodes.reserve(nNodes * 4));
    HIP_TRY(s->tlas.tlasIdx.reserve(n));
    if (s->buildScratchFor != n) {
        s->buildScratchFor = 0;
        HIP_TRY(s->buildScratch.alloc(tlas_build_scratch_bytes((uint32_t)n, &s->sortTempBytes)));
        s->buildScratchFor = n;
    }
    const float* xf = nullptr;
    if (transforms) {
        if (onDevice) xf = (const float*)transforms;
        else {
            HIP_TRY(s->tlas.xformStage.reserve(n * 16));   // (tbvh_update_tlas may have grown the instance array since the last rebuild)
            HIP_TRY(hipMemcpyAsync(s->tlas.xformStage, transforms, n * 64, hipMemcpyHostToDevice, c->stream));
            xf = s->tlas.xformStage;
        }
    }
    if (s->tlas.tlasBuilder == 2) {
        if (n > 0x3fffffffull) return fail(TBVH_E_INVALID, "tbvh_rebuild_tlas_device: %llu instances: the SAH builder takes at most 2^30 - 1", (unsigned long long)n);
        if (s->tlas.tlasSahFor != n) {
            s->tlas.tlasSahFor = 0;
            HIP_TRY(s->tlas.tlasSah.alloc(sah_scratch_bytes((uint32_t)n, &s->tlas.tlasSahSort, &s->tlas.tlasSahScan)));
            HIP_TRY(s->tlas.tlasWald.alloc(n * 4));
            s->tlas.tlasSahFor = n;
        }
        // the existing instance update, the reference's BVH::Build( BLASInstance*, n ) over the updated records, BVH_GPU::ConvertFrom: all on the stream
        HIP_TRY(timedBegin(c));
        HIP_TRY(launch_tlas_instance_update(s->tlas.instances, xf, s->tlas.blasBounds, (uint32_t)n, (uint32_t)s->tlas.nBlas, s->buildScratch, s->sortTempBytes, c->stream));
        uint32_t nWald = 0;
        HIP_TRY(run_sah_build(SahSrc(sah_boxes_instances(s->tlas.instances.get())), (uint32_t)n, 0, c->sahSmallSubtree, c->sahOneGroup, s->tlas.tlasWald, s->tlas.tlasIdx, s->tlas.tlasSah,
                              s->tlas.tlasSahSort, s->tlas.tlasSahScan, c->status, c->stream, &nWald));
        HIP_TRY(run_al_encode(s->tlas.tlasWald, nWald, (uint32_t)n, s->tlas.tlasSah, s->tlas.tlasSahSort, s->tlas.tlasSahScan, s->nodes, c->stream));
        s->tlas.nTlasNodes = nWald - 1; s->tlas.nTlasIdx = n;
        if (int r = buildWideTlas(s)) return r;
        HIP_TRY(timedEnd(c));
        return 0;
    }
    HIP_TRY(timedBegin(c));
    HIP_TRY(launch_tlas_rebuild(s->nodes, s->tlas.tlasIdx, s->tlas.instances, xf, s->tlas.blasBounds, (uint32_t)n, (uint32_t)s->tlas.nBlas, s->buildScratch, s->sortTempBytes, c->stream));
    s->tlas.nTlasNodes = nNodes; s->tlas.nTlasIdx = n;
    if (int r = buildWideTlas(s)) return r;
    HIP_TRY(timedEnd(c));
    return 0;
}

int tbvh_tlas_set_builder(tbvh_scene* s, int builder) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_tlas_set_builder");
    if (!s || !s->isTlas) return fail(TBVH_E_INVALID, "tbvh_tlas_set_builder: not a TLAS");
    if (builder != 0 && builder != 2) return fail(TBVH_E_INVALID, "tbvh_tlas_set_builder: builder %d (0 = LBVH, 2 = the reference's SAH tree)", builder);
    TBVH_LOCK(s->ctx);
    s->tlas.tlasBuilder = builder;
    return 0;
}

int tbvh_tlas_download(tbvh_scene* s, void* nodes64, uint64_t capNodes, uint32_t* idx, uint64_t capIdx, void* instances192, uint64_t capInst,
                       uint64_t* nNodesOut) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_tlas_download");
    if (!s || !s->isTlas) return fail(TBVH_E_INVALID, "tbvh_tlas_download: not a TLAS");
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t n = s->tlas.nInst, nNodes = s->tlas.nTlasNodes;
    if (nNodesOut) *nNodesOut = nNodes;
    if (nodes64) { if (capNodes < nNodes) return fail(TBVH_E_INVALID, "tbvh_tlas_download: node buffer too small"); HIP_TRY(hipMemcpy(nodes64, s->nodes, nNodes * 64, hipMemcpyDeviceToHost)); }
    if (idx) { if (capIdx < n) return fail(TBVH_E_INVALID, "tbvh_tlas_download: index buffer too small"); HIP_TRY(hipMemcpy(idx, s->tlas.tlasIdx, n * 4, hipMemcpyDeviceToHost)); }
    if (instances192) { if (capInst < n) return fail(TBVH_E_INVALID, "tbvh_tlas_download: instance buffer too small"); HIP_TRY(hipMemcpy(instances192, s->tlas.instances, n * 192, hipMemcpyDeviceToHost)); }
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
        mine.swap(s->tlas.blasList);
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
// (the lock: the number follows the scene's wide copies, which queries on other threads make and free)
uint64_t tbvh_scene_device_bytes(const tbvh_scene* s) {
    if (!s) return 0;
    TBVH_LOCK(s->ctx);
    return sceneBytes(s);
}

int tbvh_debug_scene_bytes(const tbvh_scene* s, uint64_t out[8]) {
    if (!s || !out) return fail(TBVH_E_INVALID, "tbvh_debug_scene_bytes: null argument");
    TBVH_LOCK(s->ctx);
    const SceneBytes b = sceneBytesByWord(s);
    std::memcpy(out, b.word, sizeof b.word);
    return 0;
}

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
    if (v != 0 && s->triTest) return fail(TBVH_E_INVALID, "tbvh_set_variant: the scene is in watertight mode (tbvh_set_triangle_test); the pinned kernels have no watertight form");
    const bool viewChanges = !s->isTlas && s->copies.live() && (s->variant == 0) != (v == 0);
    s->variant = v;
    if (viewChanges) return refreshBlasDescs(s);   // (the TLASes over this BLAS enter it through the copy, or through its own nodes)
    return 0;
}
}  // extern "C"
