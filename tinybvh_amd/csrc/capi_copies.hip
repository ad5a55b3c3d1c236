// capi_copies.hip — what the library derives from a scene's arrays and keeps beside them: the wide copies of a BLAS in another layout (WideCopies) and
// the re-layouts of a BVH8_CWBVH scene's own arrays (CwbvhLayouts).  Everything that makes, drops, refits or selects one is here; WHEN the wide copies
// go and come back is CopyPolicy's arithmetic (copy_policy.h).  The owner's bytes count them all, as they are when asked (capi_scene.hip: sceneBytes).
#include "capi_internal.h"

using namespace tbvh;
using namespace tbvh_capi;

namespace tbvh_capi {
// ---- re-layouts of a BVH8_CWBVH scene -----------------------------------------------------------------------------------------------------
// A BVH8_CWBVH scene whose node array is larger than twice the 256 MB Infinity Cache is traversed through a copy with one node per
// 128-byte line: an 80-byte node straddles 1.6 lines on average, and once the lines come from HBM that is 17 % more traffic than the
// 60 % larger array costs (tools/size_sweep.py, 60 M triangles: bounce rays +6 %; below that size the smaller footprint wins).
static int padCwbvhIfLarge(tbvh_scene* s) {
    if (s->layout != TBVH_LAYOUT_CWBVH || s->isTlas || s->cw.padded || (uint64_t)s->nNodes * 80 < (512ull << 20)) return 0;
    if ((uint64_t)s->nNodes * 8 >> 32) return 0;   // (cw_load_node addresses float4s with 32 bits: beyond 2^29 nodes — 64 GB padded — the packed array serves)
    tbvh_context* c = s->ctx;
    if (s->cw.padded.alloc((size_t)s->nNodes * 8) != hipSuccess) { (void)hipGetLastError(); return 0; }   // no memory to spare: the packed array serves
    launch_cwbvh_pad(s->nodes, s->cw.padded, s->nNodes, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int resetCwbvhLayouts(tbvh_scene* s, bool levelOrder) {
    s->cw.padded.reset(); s->cw.hybrid.reset(); s->cw.trisPadded.reset(); s->cw.perm.reset();
    s->cw.packed = 0; s->cw.tried = false; s->cw.levelOrder = levelOrder;
    return padCwbvhIfLarge(s);   // (padded nodes now, the incoherent-batch copies lazily)
}

static size_t hybridBlocks(uint32_t nNodes, uint32_t K) { return (size_t)K * 5 + (size_t)(nNodes - K) * 8; }   // 16-byte blocks of the hybrid node copy
static size_t hybridBytes(uint32_t nNodes, uint32_t K) { return hybridBlocks(nNodes, K) * 16; }

// the triangles the hybrid copy embeds, one in the spare 48 bytes of each node's line (TBVH_EMBED_TRIS=0 / experiment flag 8: none)
static const float4* embeddedTris(const tbvh_scene* s) { return (s->ctx->embedTris && !(s->ctx->expFlags & 8u)) ? s->tris.get() : nullptr; }

int rederiveCwbvhLayouts(tbvh_scene* s) {
    hipStream_t st = s->ctx->stream;
    if (s->cw.padded) launch_cwbvh_pad(s->nodes, s->cw.padded, s->nNodes, st);
    if (s->cw.hybrid) launch_cwbvh_derive_hybrid(s->nodes, s->cw.perm, s->cw.hybrid, s->nNodes, s->cw.packed, embeddedTris(s), st);
    if (s->cw.trisPadded) launch_cwbvh_pad_tris(s->tris, s->cw.trisPadded, s->nTriBlocks / 3, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The hybrid copy's numbering: position of every node in surface-area priority order, on the device (the stream is idle).  An array in level order needs
// none.  0, a TBVH_E_* code, or one of these two, which the lazy build takes quietly and tbvh_cwbvh_set_hybrid reports:
enum { kOrderNotATree = 1, kOrderNoMemory = 2 };
static int ensureHybridOrder(tbvh_scene* s) {
    if (s->cw.levelOrder || s->cw.perm) return 0;
    std::vector<Vec4> host((size_t)s->nNodes * 5);
    HIP_TRY(hipMemcpy(host.data(), s->nodes, host.size() * 16, hipMemcpyDeviceToHost));
    std::vector<uint32_t> perm;
    if (!cwbvh_priority_order(host.data(), s->nNodes, perm)) return kOrderNotATree;
    if (s->cw.perm.alloc(s->nNodes) != hipSuccess) { (void)hipGetLastError(); return kOrderNoMemory; }
    HIP_TRY(hipMemcpy(s->cw.perm, perm.data(), (size_t)s->nNodes * 4, hipMemcpyHostToDevice));
    return 0;
}

// BVH8_CWBVH scenes of the class that gets the per-launch coherence probe (48 - 384 MB of blobs: beyond the L2s, within reach of the Infinity
// Cache) keep two derived copies for INCOHERENT batches (kernels_cwbvh.hip: PROBED == 2): the nodes in surface-area priority order with the
// first kHybridPacked packed and the others one per 128-byte line (each with one of its triangles in the line's spare 48 bytes), and the
// triangle records padded to 64 bytes.  Built LAZILY by the first launch that would use them (capi_query.hip: planLaunch, a `probed` batch) — a
// scene that is only ever a BLAS under a TLAS, or only traced with small batches, never pays the 2.3 x memory and the host pass; that first
// launch waits for the build (~0.1 s for 600 k nodes: the node array is read back, ordered on the host, scattered on the device).  Trees made
// on the device (tbvh_convert_bvh2_device, tbvh_build_device) are in level order, which already is close to priority order: no renumbering.
// A blob that is not a strict tree (cwbvh_priority_order), one with 2^27 triangle records or more, or a failed allocation is not an error:
// the scene then runs the one-kernel path.  TBVH_INCOHERENT_COPIES=0 turns the copies off.
constexpr uint32_t kHybridPacked = 8192;
static bool wantsIncoherentCopies(const tbvh_scene* s) {
    const uint64_t blobBytes = (s->nNodeBlocks + s->nTriBlocks) * 16;
    return s->layout == TBVH_LAYOUT_CWBVH && !s->isTlas && s->ctx->incoherentCopies && blobBytes >= (48ull << 20) && blobBytes <= (384ull << 20) && s->nNodes > kHybridPacked &&
           s->nTriBlocks != 0 && s->nTriBlocks / 3 < (1ull << 27);
}
int prepareIncoherentCopies(tbvh_scene* s) {
    tbvh_context* c = s->ctx;
    if (s->cw.tried) return 0;
    s->cw.tried = true;
    if (!wantsIncoherentCopies(s)) return 0;
    const uint32_t K = kHybridPacked;
    const uint64_t nT = s->nTriBlocks / 3;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int r = ensureHybridOrder(s)) return r < 0 ? r : 0;   // (not a strict tree, no memory: traversed as uploaded)
    if (!s->cw.hybrid && s->cw.hybrid.alloc(hybridBlocks(s->nNodes, K)) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (!s->cw.trisPadded && s->cw.trisPadded.alloc(nT * 4) != hipSuccess) { (void)hipGetLastError(); s->cw.hybrid.reset(); return 0; }
    s->cw.packed = K;
    HIP_TRY(hipMemsetAsync(s->cw.hybrid, 0, hybridBytes(s->nNodes, K), c->stream));
    if (int r = rederiveCwbvhLayouts(s)) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// order-dependent hash of what the hybrid copy's numbering depends on: which slots of every node are interior children and where they start
uint64_t cwbvhTopologyHash(const Vec4* nodes, uint32_t nNodes) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ nNodes;
    for (uint32_t i = 0; i < nNodes; i++) {
        uint32_t w[2];
        std::memcpy(&w[0], &nodes[(size_t)i * 5].w, 4); std::memcpy(&w[1], &nodes[(size_t)i * 5 + 1].x, 4);
        const uint64_t k = ((uint64_t)(w[0] >> 24) << 32) | ((w[0] >> 24) ? w[1] : 0u);
        h = (h ^ k) * 0x100000001B3ull; h ^= h >> 29;
    }
    return h;
}

// ---- wide copies of a BLAS ------------------------------------------------------------------------------------------------------------------
// TBVH_WIDE_COPY_MIN: blob entries / triangles from which a scene gets copies (0 = never), or `whenUnset`
static uint64_t wideCopyMin(uint64_t whenUnset) {
    const char* e = getenv("TBVH_WIDE_COPY_MIN");
    if (!e) return whenUnset;
    const long long v = atoll(e);
    return v <= 0 ? ~0ull : (uint64_t)v;
}

void freeCopy(tbvh_scene* s, CopyKind kind) {
    if (!s) return;
    tbvh_scene*& slot = kind == kCopyWide4 ? s->copies.copy4 : s->copies.copy8;
    tbvh_scene* w = slot;
    if (!w) return;
    slot = nullptr;
    tbvh_free_scene(w);   // (the opacity maps it read are the owner's: tbvh_scene::opmapOwn)
}

// The 8-wide copy of a BVH_GPU / BVH4_GPU scene, made LAZILY by the scene's first query of 1024 rays or more (capi_query.hip: prepareScene) — a BLAS
// that is only ever traced through a TLAS never pays for it — from what the scene keeps on the device: the blob is read back, the host turns it into a
// Wald-layout BVH2 with leaves of at most 3 entries (host_builder.cpp: bvh_gpu_to_bvh2 in record mode / bvh4_gpu_to_bvh2), the device converter every
// BVH8_CWBVH conversion uses collapses and encodes it in ITS record mode (kernels_convert.hip; the greedy collapse of MBVH<8>::ConvertFrom,
// tiny_bvh.h:4975-5048): triangle records are carried over bit for bit.  Blobs below TBVH_WIDE_COPY_MIN entries / triangles (default 32768; 0 = never)
// keep their own kernel.  A failure here is never an error of the query: the scene then simply traces its own nodes.
// One copy of scene s in the `target` layout (BVH8_CWBVH from a BVH_GPU / BVH4_GPU scene, BVH4_GPU from a BVH_GPU / BVH8_CWBVH one), or nullptr (too small,
// too large, out of memory: never an error of the caller's operation).  Not listed in the context's scene table; shares the owner's opacity maps.
// forTlas: the copy is wanted by a TLAS over s — there ONE kernel class for all BLASes is worth more than any single BLAS's speed (a BLAS without the copy
// puts the whole TLAS on the flat loop), so small blobs get one too (from 64 entries; TBVH_WIDE_COPY_MIN still rules when set).
static tbvh_scene* buildCopy(tbvh_scene* s, int target, bool forTlas) {
    tbvh_context* c = s->ctx;
    // (a watertight BVH_GPU / BVH4_GPU scene has no other kernel than the 8-wide one: a copy whatever its size, whatever TBVH_WIDE_COPY_MIN says)
    const uint64_t minIdx = (s->triTest && target == TBVH_LAYOUT_CWBVH) ? 1 : wideCopyMin(forTlas ? 64 : kWideCopyMin);
    std::vector<Node2> n2;
    std::vector<Vec4> blob, recs;
    const float4* dRecs = nullptr;
    uint64_t nRecs = 0;
    DevBuf<float4> dN2, dOwnRecs;
    try {
        if (s->layout == TBVH_LAYOUT_BVH_GPU) {
            const uint64_t nNodes = s->nNodeBlocks / 4, nIdx = s->nTriBlocks / 3;
            if (nIdx < minIdx || nIdx > 0x7fffffffull || nNodes > 0x3fffffffull) return nullptr;
            blob.resize(s->nNodeBlocks); recs.resize(s->nTriBlocks);
            if (hipMemcpyAsync(blob.data(), s->nodes, s->nNodeBlocks * 16, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                hipMemcpyAsync(recs.data(), s->tris, s->nTriBlocks * 16, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            if (!bvh_gpu_to_bvh2((const NodeAL*)blob.data(), nNodes, nullptr, nIdx, nullptr, 0, 3u, n2, recs.data())) return nullptr;
            dRecs = s->tris; nRecs = nIdx;       // (the gathered records are on the device already, in leaf order)
        } else {
            if (s->layout == TBVH_LAYOUT_BVH4_GPU) {
                if (s->nNodeBlocks / 4 < minIdx || s->nNodeBlocks > 0x7fffffffull) return nullptr;   // (a stream of n triangles has at least 3 n blocks: a cheap first cut)
                blob.resize(s->nNodeBlocks);
                if (hipMemcpyAsync(blob.data(), s->nodes, s->nNodeBlocks * 16, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                    hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
                if (!bvh4_gpu_to_bvh2(blob.data(), s->nNodeBlocks, 3u, n2, recs)) return nullptr;
            } else {   // BVH8_CWBVH
                if (s->nTriBlocks / 3 < minIdx || s->nTriBlocks > 0x7fffffffull) return nullptr;
                std::vector<Vec4> tris(s->nTriBlocks);
                blob.resize(s->nNodeBlocks);
                if (hipMemcpyAsync(blob.data(), s->nodes, s->nNodeBlocks * 16, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                    hipMemcpyAsync(tris.data(), s->tris, s->nTriBlocks * 16, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                    hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
                if (!cwbvh_to_bvh2(blob.data(), s->nNodeBlocks / 5, tris.data(), s->nTriBlocks, n2, recs)) return nullptr;
            }
            nRecs = recs.size() / 3;
            if (nRecs < minIdx || nRecs > 0x7fffffffull) return nullptr;
            if (dOwnRecs.alloc(recs.size()) != hipSuccess ||
                hipMemcpyAsync(dOwnRecs, recs.data(), recs.size() * 16, hipMemcpyHostToDevice, c->stream) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            dRecs = dOwnRecs;
        }
    } catch (const std::bad_alloc&) { return nullptr; }
    if (n2.size() > 0x7fffffffull) return nullptr;
    if (dN2.alloc(n2.size() * 2) != hipSuccess ||
        hipMemcpyAsync(dN2, n2.data(), n2.size() * 32, hipMemcpyHostToDevice, c->stream) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    tbvh_scene* w = nullptr;
    if (convertDeviceImpl(c, target, dN2, n2.size(), nullptr, nRecs, flat_mesh(dRecs, nRecs), &w) != 0 || !w) { (void)hipGetLastError(); return nullptr; }
    for (size_t i = 0; i < c->scenes.size(); i++)
        if (c->scenes[i] == w) { c->scenes.erase(c->scenes.begin() + i); break; }   // owned by `s`, freed with it
    w->opmap = s->opmap; w->opmapN = s->opmapN;
    return w;
}

// What a TLAS traverses for BLAS b is tlas_plan.h's rule (sentences 1 - 4) over these facts; the numbers behind it (1000 instances of a 100 k-triangle BLAS,
// camera / shadow / random MRays/s) are in DESIGN.md par. 3.5: k_tlas4 is the fastest two-level kernel for closest hits, k_tlas8 for any-hit queries.
TlasBlasFacts tlasBlasFacts(const tbvh_scene* b) {
    TlasBlasFacts f;
    f.layout = b->layout; f.pinned = b->variant != 0; f.has8 = b->copies.copy8 != nullptr; f.has4 = b->copies.copy4 != nullptr; f.watertight = b->triTest != 0;
    return f;
}
const tbvh_scene* blasView(const tbvh_scene* b, TlasView v) { return v == kViewWide4 ? b->copies.copy4 : v == kViewWide8 ? b->copies.copy8 : b; }

// the 8-wide copy is of a BVH_GPU / BVH4_GPU scene, the 4-wide one of a BVH_GPU / BVH8_CWBVH one and always for the TLASes over it
static bool layoutHasCopy(const tbvh_scene* s, CopyKind kind) {
    return s->layout == TBVH_LAYOUT_BVH_GPU || s->layout == (kind == kCopyWide4 ? TBVH_LAYOUT_CWBVH : TBVH_LAYOUT_BVH4_GPU);
}

// (one body for what were makeWideCopy and makeWide4Copy)
static int makeCopy(tbvh_scene* s, CopyKind kind) {
    const bool four = kind == kCopyWide4;
    freeCopy(s, kind);
    (four ? s->copies.tried4 : s->copies.tried8) = true;
    const bool has = !s->isTlas && layoutHasCopy(s, kind);
    if (tbvh_scene* w = has ? buildCopy(s, four ? TBVH_LAYOUT_BVH4_GPU : TBVH_LAYOUT_CWBVH, four || !s->usedBy.empty()) : nullptr) {
        (four ? s->copies.copy4 : s->copies.copy8) = w;
        if (!four) {
            // a copy below the size at which the scene's OWN queries gain from it (made for the TLASes over the scene): those queries keep the uploaded nodes
            const uint64_t entries = s->layout == TBVH_LAYOUT_BVH_GPU ? s->nTriBlocks / 3 : w->nTriBlocks / 3;
            s->copies.tlasOnly = entries < kWideCopyMin && wideCopyMin(0) == 0 && !s->triTest;   // (0: the variable is not set)
            shareTriangleTest(s);
        }
    }
    forEachTlasOver(s, [](tbvh_scene* t) { (void)reclassifyTlas(t); return 0; });   // (the copy's arrays are new ones — or gone)
    return 0;
}

void makeCopyOnce(tbvh_scene* b, CopyKind kind) {
    if (layoutHasCopy(b, kind) && !(kind == kCopyWide4 ? b->copies.tried4 : b->copies.tried8) && b->variant == 0) makeCopy(b, kind);
}

int ensureWatertightCopy(tbvh_scene* s) {
    if (!s->triTest || s->isTlas || !layoutHasCopy(s, kCopyWide8)) return 0;
    if (!s->copies.copy8) makeCopy(s, kCopyWide8);
    if (!s->copies.copy8)
        return fail(TBVH_E_INVALID, "a watertight BVH_GPU / BVH4_GPU scene is traced through its 8-wide copy, and none could be made (a blob whose root is a leaf, or no memory)");
    s->copies.tlasOnly = false;
    shareTriangleTest(s);
    return 0;
}

void dropCopiesAfterUpdate(tbvh_scene* s) {
    const uint8_t live = s->copies.live();
    if (!(live | s->copies.pending())) return;
    s->copies.policy.dropped(live);
    hipStreamSynchronize(s->ctx->stream);
    freeCopy(s, kCopyWide8); freeCopy(s, kCopyWide4);
    forEachTlasOver(s, [](tbvh_scene* t) { (void)reclassifyTlas(t); t->tlas.blasRecopyPending = true; return 0; });   // (the TLASes enter this BLAS through its own nodes meanwhile)
}

// one query on BLAS b (or through a TLAS over it) since its copies were dropped: they come back once the blob has settled
static void countQueryOn(tbvh_scene* b) {
    const uint8_t kinds = b->copies.policy.query();
    if (kinds & kCopyWide8) makeCopy(b, kCopyWide8);
    if (kinds & kCopyWide4) makeCopy(b, kCopyWide4);
}

void countQueryForRecopy(tbvh_scene* s) {
    if (!s->isTlas) { if (s->copies.pending()) countQueryOn(s); return; }
    if (!s->tlas.blasRecopyPending) return;
    bool still = false;
    for (tbvh_scene* b : s->tlas.blasList)
        if (b->copies.pending()) { countQueryOn(b); still |= b->copies.pending() != 0; }
    s->tlas.blasRecopyPending = still;
}

tbvh_scene* wideCopyForQuery(tbvh_scene* s) { return s->variant == 0 && !s->copies.tlasOnly ? s->copies.copy8 : nullptr; }
tbvh_scene* tunedScene(tbvh_scene* s) { return s->copies.copy8 ? s->copies.copy8 : s; }

void shareOpacityMaps(tbvh_scene* s) {
    for (tbvh_scene* w : {s->copies.copy8, s->copies.copy4})
        if (w) { w->opmap = s->opmap; w->opmapN = s->opmapN; }   // (shared, owned by s)
}

// a mesh refitted every frame with few rays traced in between: the copies are dropped (they come back like after an update); otherwise they follow, from the
// same vertices, already on the device
int refitCopies(tbvh_scene* s, const MeshSrc& src) {
    uint64_t total = s->raysTraced;
    forEachTlasOver(s, [&](tbvh_scene* t) { total += t->raysTraced; return 0; });
    if (s->copies.policy.refit(total, s->copies.live() != 0)) { dropCopiesAfterUpdate(s); return 0; }
    if (s->copies.copy8) if (int r = refitDeviceSource(s->copies.copy8, src)) return r;
    if (s->copies.copy4) return refitDeviceSource(s->copies.copy4, src);
    return 0;
}
}  // namespace tbvh_capi

extern "C" int tbvh_cwbvh_set_hybrid(tbvh_scene* s, int64_t packedNodes) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_cwbvh_set_hybrid");
    TBVH_REFUSE_VOXEL(s, "tbvh_cwbvh_set_hybrid");
    TBVH_REFUSE_CUSTOM(s, "tbvh_cwbvh_set_hybrid");
    if (!s || s->isTlas || s->layout != TBVH_LAYOUT_CWBVH) return fail(TBVH_E_INVALID, "tbvh_cwbvh_set_hybrid: not a BVH8_CWBVH scene");
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    s->cw.hybrid.reset();
    s->cw.tried = true;   // the caller decides now: no lazy build behind its back
    if (packedNodes < 0) return 0;
    if (s->nTriBlocks / 3 >= (1ull << 27)) return fail(TBVH_E_INVALID, "tbvh_cwbvh_set_hybrid: 2^27 triangle records or more");
    if ((uint64_t)s->nNodes * 8 >> 32) return fail(TBVH_E_INVALID, "tbvh_cwbvh_set_hybrid: 2^29 nodes or more (the copy is addressed in 32-bit float4 offsets: cwbvh_node.h)");
    const uint32_t K = (uint32_t)std::min<uint64_t>((uint64_t)packedNodes, s->nNodes) & ~7u;   // the padded part starts on a 128-byte line
    if (int r = ensureHybridOrder(s)) {
        if (r == kOrderNotATree) return fail(TBVH_E_FORMAT, "tbvh_cwbvh_set_hybrid: the node array is not a strict tree (a child range shared by two parents or out of range)");
        return r == kOrderNoMemory ? fail(TBVH_E_HIP, "tbvh_cwbvh_set_hybrid: no device memory for the node order") : r;
    }
    HIP_TRY(s->cw.hybrid.alloc(hybridBlocks(s->nNodes, K)));
    HIP_TRY(hipMemsetAsync(s->cw.hybrid, 0, hybridBytes(s->nNodes, K), c->stream));
    s->cw.packed = K;
    if (!s->cw.trisPadded && s->nTriBlocks) {
        const uint64_t nT = s->nTriBlocks / 3;
        HIP_TRY(s->cw.trisPadded.alloc(nT * 4));
    }
    if (int r = rederiveCwbvhLayouts(s)) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}
