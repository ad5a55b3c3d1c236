// capi_query.hip — the query path: launchQuery and its steps (the plan of launch_plan.h carried out: lane, counter pool, probe, kernels), host-array
// staging, multi-device sharding, ray generators.
#include "capi_internal.h"
#include "voxel_edit.h"

using namespace tbvh;
using namespace tbvh_capi;

namespace tbvh_capi {
int ensureStage(tbvh_context* c, uint64_t n) {
    HIP_TRY(c->stageRays.reserve(n));
    return 0;
}
int ensureStageOcc(tbvh_context* c, uint64_t n) {
    HIP_TRY(c->stageOcc.reserve(n));
    return 0;
}
}  // namespace tbvh_capi

void CohTuner::harvest(float minMs) {
    for (size_t k = 0; k < pending.size();) {
        const Pending pe = pending[k];
        const hipError_t qe = hipEventQuery(pe.e1);
        if (qe == hipErrorNotReady) { (void)hipGetLastError(); k++; continue; }
        float t1 = 0.f;
        if (qe == hipSuccess && hipEventElapsedTime(&t1, pe.e0, pe.e1) == hipSuccess && t1 > minMs) {
            // time per ray depends on the batch size (the tail of a launch): only batches of about one size are compared
            if (!refRays) refRays = pe.rays;
            if (pe.rays * 4 >= refRays * 3 && pe.rays * 3 <= refRays * 4) {
                const float perRay = t1 * 1e6f / (float)pe.rays;
                n[pe.mode - 1]++;
                if (perRay < best[pe.mode - 1]) best[pe.mode - 1] = perRay;
            }
        } else (void)hipGetLastError();
        hipEventDestroy(pe.e0); hipEventDestroy(pe.e1);
        pending.erase(pending.begin() + k);
    }
}

void CohTuner::settle(bool packetOrStrict, float margin) {
    if (n[0] >= kSamples && n[1] >= kSamples && n[2] >= kSamples) {
        int win = 0;   // the deferred + gated schedule unless another one beats it by 3 %
        for (int m = 1; m < kModes; m++) if (best[m] < 0.97f * best[0] && best[m] < best[win]) win = m;
        if (packetOrStrict) {   // strict (= from now on the unprobed single kernel) unless the packet kernel wins by the margin AND by more than the second launch costs
            const float gainMs = (best[1] - best[2]) * (float)refRays * 1e-6f;
            win = (best[2] < margin * best[1] && gainMs >= 0.015f) ? 2 : 1;
        }
        decided = win + 1; drop_pending();
    } else if (launches >= 96) { decided = 1; drop_pending(); }   // batches too varied to compare: the schedule that wins on most scenes
}

int CohTuner::least_sampled() const {
    uint32_t cnt[kModes];
    for (int m = 0; m < kModes; m++) cnt[m] = n[m];
    for (const Pending& pe : pending) cnt[pe.mode - 1]++;
    int least = 0;
    for (int m = 1; m < kModes; m++) if (cnt[m] < cnt[least]) least = m;
    return least;
}

namespace tbvh_capi {

int ensurePipe(tbvh_context* c, uint64_t nHits) {
    if (!c->pipe) {
        // built aside and published only when complete: a failure half way (pinned memory is a scarce resource) must leave the context without a
        // pipe, so that the next host query tries again instead of running on null buffers (HIP_TRY returns; ~HostPipe releases what was made)
        std::unique_ptr<HostPipe> p(new (std::nothrow) HostPipe);
        if (!p) return fail(TBVH_E_NOMEM, "out of host memory");
        for (int i = 0; i < 2; i++) {
            HIP_TRY(hipHostMalloc(&p->pinUp[i], HostPipe::kChunk * 64, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&p->evUp[i], hipEventDisableTiming));
        }
        HIP_TRY(hipStreamCreateWithFlags(&p->down, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&p->evKernel, hipEventDisableTiming));
        // The packing and scattering of the caller's records is host memcpy work: 16.7 M records of a tinybvh::Ray[] pack in 78 / 22 / 17 / 13 ms on
        // 1 / 4 / 8 / 16 threads of the round-5 box (tools/ubench/link_rate.hip) against 19 ms the link needs for them — every core the process
        // may use takes part (up to 16), the calling thread being one of them
        const uint32_t hw = usable_host_threads();
        uint32_t t = hw > 16 ? 15 : hw > 1 ? hw - 1 : 0;
        if (const char* e = getenv("TBVH_HOST_THREADS")) { const int v = atoi(e); if (v >= 1 && v <= 64) t = (uint32_t)v - 1; }
        try { p->start(t); }
        catch (const std::exception&) { return fail(TBVH_E_NOMEM, "cannot start the host staging threads"); }   // (~HostPipe joins the ones that did start)
        c->pipe = p.release();
    }
    HostPipe* p = c->pipe;
    if (p->packed.count() < nHits * 5) {   // nHits: 20-byte result records the two buffers must hold (two groups of a closest-hit batch, or an any-hit batch's flags)
        HIP_TRY(hipStreamSynchronize(p->down));
        p->packed.reset();   // (a failure below leaves no device buffer: the next query makes both again)
        if (p->pinDown) hipHostFree(p->pinDown);
        p->pinDown = nullptr;
        HIP_TRY(hipHostMalloc(&p->pinDown, nHits * 20, hipHostMallocDefault));
        HIP_TRY(p->packed.alloc(nHits * 5));
    }
    return 0;
}

static bool isPinned(tbvh_context* c, const void* p, uint64_t bytes) {
    for (const tbvh_context::PinnedRange& r : c->pinned)
        if ((const char*)p >= r.host && (const char*)p + bytes <= r.host + r.bytes) return true;
    return false;
}

// ---- a host ray array through the device, pipelined -----------------------------------------------------------------------------------------
// tiny_bvh_speedtest.cpp:1110-1137 does, one after the other: a memcpy loop (64 of every 128 bytes into a tinyocl::Buffer), CopyToDevice, Kernel::Run,
// CopyFromDevice, and the caller's loop over the results.  Here the batch is cut into groups of ~4 M rays and the stages of consecutive groups
// overlap: while the host threads pack group g + 1 into the pinned upload ring (chunks of 256 k rays, two buffers) and the link carries them up,
// the device traces group g and a second stream packs its 20 result bytes per ray and carries them DOWN (the link is full duplex:
// 48 GB/s each way at once against 57 one way, tools/ubench/link_rate.hip); the host scatters group g - 1's results into the caller's records.
// What was measured and NOT taken (profiles/r05_link_rate.txt): hipMemcpy2D for the strided side (19 GB/s up, 3-4 GB/s down), and the device
// reading / writing the caller's pinned array itself (a 128-byte record costs a 128-byte read for its 64 useful bytes: 27 GB/s; 20-byte writes
// cost a 64-byte line each: 20 GB/s of results).  A packed (64-byte) array in page-locked memory of the library's (tbvh_pinned_malloc) needs no packing: it goes up
// by DMA straight from there.
// Groups of ~1 M rays (round 6; 4 M before): the first group's packing and the last group's scatter overlap with nothing, so the smaller the group
// the shorter the pipeline's fill and drain (~3 ms each of a 34 ms call at 4 M); a 1 M-ray launch still runs at > 3 GRays/s, far above the link.
// The result buffers (device: packed hits, host: pinned) hold TWO groups and are used alternately — group g's results land in one while the host
// scatters group g - 1 out of the other (16.7 M rays: 2 x 21 MB page-locked where the whole batch took 335 MB).
constexpr uint64_t kGroupRays = 1ull << 20;
constexpr uint64_t kDirectRays = 16384;   // batches up to this size skip the pipeline (no worker threads, no pinned ring): two strided copies around the launch

// a small host batch: strided copy up, launch, strided copy of bytes 44..63 back; synchronous
static int hostQuerySmall(tbvh_scene* s, const char* raysIn, char* raysOut, uint64_t n, uint32_t stride, uint8_t* occ) {
    tbvh_context* c = s->ctx;
    if (int r = ensureStage(c, n)) return r;
    if (occ) if (int r = ensureStageOcc(c, n)) return r;
    HIP_TRY(hipMemcpy2DAsync(c->stageRays, 64, raysIn, stride, 64, n, hipMemcpyHostToDevice, c->stream));
    if (int r = launchQuery(s, c->stageRays, n, occ ? c->stageOcc : nullptr)) return r;
    if (occ) HIP_TRY(hipMemcpyAsync(occ, c->stageOcc, n, hipMemcpyDeviceToHost, c->stream));
    else HIP_TRY(hipMemcpy2DAsync(raysOut + 44, stride, (const char*)c->stageRays.get() + 44, 64, 20, n, hipMemcpyDeviceToHost, c->stream));
    return checkStatus(c);   // (synchronizes the stream)
}

int hostQuery(tbvh_scene* s, const char* raysIn, char* raysOut, uint64_t n, uint32_t stride, uint8_t* occ) {
    tbvh_context* c = s->ctx;
    if (n <= kDirectRays) return hostQuerySmall(s, raysIn, raysOut, n, stride, occ);
    if (int r = ensureStage(c, n)) return r;
    if (occ) if (int r = ensureStageOcc(c, n)) return r;
    const uint64_t G = n <= kGroupRays + kGroupRays / 2 ? 1 : (n + kGroupRays - 1) / kGroupRays;
    const uint64_t per = (((n + G - 1) / G) + HostPipe::kChunk - 1) / HostPipe::kChunk * HostPipe::kChunk;
    if (int r = ensurePipe(c, occ ? (n + 19) / 20 : 2 * per)) return r;   // (two groups of 20-byte closest-hit records, or one byte per any-hit flag)
    HostPipe* p = c->pipe;
    const bool direct = stride == 64 && isPinned(c, raysIn, n * 64);
    while (p->evGroup.size() < G) { hipEvent_t e = nullptr; HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); p->evGroup.push_back(e); }
    const uint64_t seq0 = c->evSeq;
    uint64_t chunkNo = 0;
    auto drain = [&](uint64_t g) -> int {   // group g's results into the caller's records
        const uint64_t b = g * per, e = b + per < n ? b + per : n;
        HIP_TRY(hipEventSynchronize(p->evGroup[g]));
        const char* pin = (const char*)p->pinDown + (g & 1) * per * 20;
        p->parallel_for(e - b, [=](uint32_t part, uint32_t parts) {
            const uint64_t lo = (e - b) * part / parts, hi = (e - b) * (part + 1) / parts;
            for (uint64_t i = lo; i < hi; i++) std::memcpy(raysOut + (b + i) * stride + 44, pin + i * 20, 20);
        });
        return 0;
    };
    for (uint64_t g = 0; g < G; g++) {
        const uint64_t b = g * per, e = b + per < n ? b + per : n;
        for (uint64_t first = b; first < e; first += HostPipe::kChunk, chunkNo++) {
            const uint64_t cnt = e - first < HostPipe::kChunk ? e - first : HostPipe::kChunk;
            if (direct) { HIP_TRY(hipMemcpyAsync(c->stageRays + first, raysIn + first * 64, cnt * 64, hipMemcpyHostToDevice, c->stream)); continue; }
            const int k = (int)(chunkNo & 1);
            if (chunkNo >= 2) HIP_TRY(hipEventSynchronize(p->evUp[k]));   // the DMA that last read this buffer is done
            char* pin = (char*)p->pinUp[k];
            const char* src = raysIn + first * stride;
            p->parallel_for(cnt, [=](uint32_t part, uint32_t parts) {
                const uint64_t lo = cnt * part / parts, hi = cnt * (part + 1) / parts;
                if (stride == 64) std::memcpy(pin + lo * 64, src + lo * 64, (hi - lo) * 64);
                else for (uint64_t i = lo; i < hi; i++) std::memcpy(pin + i * 64, src + i * stride, 64);
            });
            HIP_TRY(hipMemcpyAsync(c->stageRays + first, pin, cnt * 64, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipEventRecord(p->evUp[k], c->stream));
        }
        if (int r = launchQuery(s, c->stageRays + b, e - b, occ ? c->stageOcc + b : nullptr)) return r;
        if (!occ) {
            // (the half of the result buffers this group uses was last read by drain(g - 2), which returned before this point was reached)
            uint32_t* packed = p->packed + (g & 1) * per * 5;
            HIP_TRY(hipEventRecord(p->evKernel, c->stream));
            HIP_TRY(hipStreamWaitEvent(p->down, p->evKernel, 0));
            launch_pack_hits(c->stageRays + b, packed, e - b, p->down);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync((char*)p->pinDown + (g & 1) * per * 20, packed, (e - b) * 20, hipMemcpyDeviceToHost, p->down));
            HIP_TRY(hipEventRecord(p->evGroup[g], p->down));
            if (g) if (int r = drain(g - 1)) return r;
        }
    }
    if (occ) HIP_TRY(hipMemcpyAsync(p->pinDown, c->stageOcc, n, hipMemcpyDeviceToHost, c->stream));
    else if (int r = drain(G - 1)) return r;
    if (int r = checkStatus(c)) return r;
    if (occ) std::memcpy(occ, p->pinDown, n);
    // the query's device time = the sum over its groups' launches (what tbvh_time_last_ms reports for a host-array query)
    if (!c->skipTiming && c->evSeq - seq0 == G && G <= tbvh_context::kTimeRing) {
        float sum = 0.f; bool ok = true;
        for (uint64_t q = seq0; q < c->evSeq && ok; q++) {
            const uint32_t slot = (uint32_t)(q % tbvh_context::kTimeRing);
            float t = 0.f;
            ok = c->evDone[slot] && hipEventElapsedTime(&t, c->evRing[slot][0], c->evRing[slot][1]) == hipSuccess;
            sum += t;
        }
        if (ok) { c->hostQueryMs = sum; c->hostQuerySeq = c->evSeq; } else (void)hipGetLastError();
    }
    return 0;
}

// one counter area: the pool's partitions + the coherence-probe counters on their own line
constexpr size_t kPoolWords = (size_t)(kPoolParts + 1) * kPoolCounterStride;

// One launch as the steps of launchQuery hand it on: each member is set once, by the step named.
struct Launch {
    bool any = false, overlaps = false;   // IsOccluded; it may take lane 1 and the lanes' book records it (launchQuery)
    LaneFootprint fp;                // the bytes it writes (footprintOf)
    int lane = 0;                    // chooseLane
    hipStream_t st = nullptr;        // ... and that lane's stream
    uint32_t* probeLine = nullptr;   // the coherence probe's counters in this launch's pool area (bindLanePool)
    uint64_t launchSeq = 0;          // its event pair (launchQuery, after timedBegin): the number LaneBook::gate and the verdict memory know it by,
    uint32_t ringSlot = 0;           //   and the pair's place in the ring
    ProbeKey key;                    // armProbe: the probe's verdict on this launch will be remembered under `key` (remember); the buffer's last two
    bool remember = false, solo = false;   //   finished launches were incoherent (probe_memory.h) and the coherent flavor is left out (solo)
};

static LaneFootprint footprintOf(const RayRec* d_rays, uint64_t n, const uint8_t* d_occ) {
    LaneFootprint fp;
    fp.rays.lo = (uintptr_t)d_rays; fp.rays.hi = fp.rays.lo + (uintptr_t)n * sizeof(RayRec);
    if (d_occ) { fp.occ.lo = (uintptr_t)d_occ; fp.occ.hi = fp.occ.lo + (uintptr_t)n; }
    return fp;
}

// ---- which kernels a scene's queries run, and how wide their stack entries are ---------------------------------------------------------------------
enum class KernelFamily { kBvh2, kBvh4, kCwbvh, kSphere, kVoxel, kTlasSphere, kTlas4, kTlas8, kTlasVoxel, kTlas2, kTlasFlat, kNone };
// A TLAS's family, class and descriptor table for each kind of query are its stored plan's (tlas_plan.h; capi_scene.hip: reclassifyTlas keeps it current).
static const TlasKindPlan& tlasKind(const tbvh_scene* s, bool any) { return s->tlas.plan.kind[any ? 1 : 0]; }
static const BlasDesc* tlasDesc(const tbvh_scene* s, bool any) { return any && s->tlas.plan.anyOwn ? s->tlas.blasDescAny.get() : s->tlas.blasDesc.get(); }

static KernelFamily kernelFamily(const tbvh_scene* s, bool any) {
    if (s->isTlas) {
        switch (tlasKind(s, any).family) {
        case TlasFamily::kTlasSphere: return KernelFamily::kTlasSphere;
        case TlasFamily::kTlas4: return KernelFamily::kTlas4;
        case TlasFamily::kTlas8: return KernelFamily::kTlas8;
        case TlasFamily::kTlasVoxel: return KernelFamily::kTlasVoxel;
        case TlasFamily::kTlas2: return KernelFamily::kTlas2;
        case TlasFamily::kTlasFlat: return KernelFamily::kTlasFlat;
        }
    }
    return s->layout == TBVH_LAYOUT_BVH_GPU ? KernelFamily::kBvh2 : s->layout == TBVH_LAYOUT_BVH4_GPU ? KernelFamily::kBvh4
           : s->layout == TBVH_LAYOUT_CWBVH ? KernelFamily::kCwbvh : s->layout == TBVH_LAYOUT_VOXELSET ? KernelFamily::kVoxel
           : s->layout == TBVH_LAYOUT_BVH2_WALD ? KernelFamily::kSphere /* a sphere BLAS (kernels_custom.hip) */ : KernelFamily::kNone;
}

// Stack entries per lane in the spill area, which holds spillEntries 32-bit words per lane: half as many where a family pushes 8-byte entries.
static uint32_t stackEntriesPerLane(const tbvh_scene* s, bool any, KernelFamily f) {
    const bool eightBytes = s->isTlas ? tlasKind(s, any).entryBytes == 8 : (f == KernelFamily::kCwbvh || f == KernelFamily::kSphere);
    return eightBytes ? s->ctx->spillEntries / 2 : s->ctx->spillEntries;
}

// One coherent-flavor kernel of a two-flavor launch, in the schedule the scene's tuner asks for; timed by the tuner's own events while it still measures.
static int launchCoherentFlavor(tbvh_scene* s, const QueryArgs& q, const LaunchPlan& P, const Launch& L, const float4* tris) {
    tbvh_context* c = s->ctx;
    QueryArgs qa = q;
    qa.baseBlocks = 0;   // every wave of the coherent flavor leaves unless the batch is coherent
    if (c->expFlags & 16u) qa.flags |= 16u;   // (debug flag 16: the coherent flavor takes the batch whatever the probe finds: tests put incoherent rays through it)
    // which schedule serves a coherent batch on this scene is measured, not assumed (CohTuner, capi_internal.h)
    s->cohLastClass[L.any ? 1 : 0] = (uint8_t)P.sizeClass;
    CohTuner& tu = s->cohTuner[L.any ? 1 : 0][P.sizeClass];
    const bool sizeKnown = q.nRaysDev == nullptr;   // a batch whose size only the device knows (the wavefront stages) cannot be priced per ray: the default schedule, no sample
    if (P.probedSmall && !tu.decided && tu.n[0] == 0) { tu.n[0] = CohTuner::kSamples; tu.best[0] = 1e30f; }   // (no deferred schedule there: strict or packet)
    if (!tu.decided && !c->cohTunerMode) {
        tu.harvest(P.probedSmall ? 0.015f : 0.05f);
        // (beyond 384 MB the per-lane flavor measured here walks the packed nodes; a scene with the padded node copy runs a few % faster unprobed)
        tu.settle(P.probedSmall, P.small ? 0.97f : 0.92f);
    }
    const bool measuring = !tu.decided && !c->cohTunerMode && sizeKnown;
    // while undecided: the schedule with the fewest samples taken or in flight (round-robin by launch count aliased with callers whose coherent
    // launches come every third time: one schedule got every sample, the others none, and the tuner idled into its fallback)
    int mode = c->cohTunerMode ? c->cohTunerMode : tu.decided ? tu.decided : measuring ? 1 + tu.least_sampled() : 1;
    if (P.probedSmall && mode == 1) mode = 2;
    if (sizeKnown) tu.launches++;
    if (mode == 2) qa.flags |= 32u;
    CohTuner::Pending pe{nullptr, nullptr, mode, q.nRays};
    if (measuring && tu.pending.size() < 16) {
        if (hipEventCreate(&pe.e0) != hipSuccess || hipEventCreate(&pe.e1) != hipSuccess || hipEventRecord(pe.e0, L.st) != hipSuccess) {   // no sample then
            if (pe.e0) hipEventDestroy(pe.e0);
            if (pe.e1) hipEventDestroy(pe.e1);
            pe.e0 = pe.e1 = nullptr; (void)hipGetLastError();
        }
    }
    if (mode == 3) launch_cwbvh_packet(L.any, s->nodes, s->tris, qa, c->status, P.blocks, L.st);   // one traversal per wave of 64 consecutive rays
    else launch_cwbvh(L.any, 0, s->nodes, tris, qa, c->status, mode == 2 ? P.blocksBase : P.blocks, L.st, 5, P.small, P.blocks7Cwbvh);
    const hipError_t le = hipGetLastError();
    if (pe.e0) {
        if (le == hipSuccess && hipEventRecord(pe.e1, L.st) == hipSuccess) tu.pending.push_back(pe);
        else { hipEventDestroy(pe.e0); hipEventDestroy(pe.e1); }
    }
    HIP_TRY(le);
    return 0;
}

// The scene's own kernel, as a launch without a second flavor runs it: on the padded node copy where the plan says so (launch_plan.h: autoPad)
static void launchSceneKernel(tbvh_scene* s, const QueryArgs& q, const LaunchPlan& P, const Launch& L, const float4* tris) {
    launch_cwbvh(L.any, s->variant, P.autoPad ? s->cw.padded : s->nodes, tris, q, s->ctx->status, P.blocks, L.st, P.autoPad ? 8 : 5, P.small, P.blocks7Cwbvh);
}

// The kernels of one launch on a BVH8_CWBVH scene, by the plan's shape (launch_plan.h: planShape).  A probed launch on a scene with the incoherent-batch
// copies (prepareIncoherentCopies) is TWO kernels back to back, each for one verdict of the probe; the one the verdict is not for leaves at once (~10 us).
// The coherent flavor keeps the packed arrays as uploaded (its working set lives in the L2s); the incoherent one walks the hybrid node copy and the
// 64-byte triangle records.
// Bistro stand-in, 16.7 M rays, interleaved medians (profiles/r03_ab_16m.txt): bounce rays +10 %, camera and shadow rays unchanged.
static int launchCwbvhKernels(tbvh_scene* s, QueryArgs& q, const LaunchPlan& P, const Launch& L) {
    tbvh_context* c = s->ctx;
    const float4* tris = s->tris;
    if (P.watertight) {   // the scene's test is the watertight one: its instantiations of the per-lane kernel, and no other (a missing vertex array is an error, never another kernel)
        if (!s->wtVerts) return fail(TBVH_E_INVALID, "a scene in watertight mode without its vertices");
        QueryArgs qw = q;
        qw.wtVerts = s->wtVerts; qw.wtTris = (uint32_t)s->wtTris;   // (in the place of stats and hybridK: device_common.h)
        // the split-ray forms (batches below 12 M rays) hold 5 waves per SIMD: a persistent grid beyond 20 workgroups per CU would only queue the rest up as a tail
        const uint32_t resident = (uint32_t)c->numCUs * 4u * kWatertightWavesPerSimd;
        const uint32_t blocksWt = (split_rays_wanted(qw) && !c->gridOverride && P.blocksBase > resident) ? resident : P.blocksBase;
        launch_cwbvh_watertight(L.any, s->nodes, s->tris, qw, c->status, blocksWt, L.st);
        return 0;
    }
#ifdef TBVH_EXPERIMENTS
    if ((c->expFlags & 2u) && s->cw.trisPadded) { tris = s->cw.trisPadded; q.flags |= 2u; }   // experiment: 64-byte triangle records in the ordinary kernels too
#endif
    switch (P.shape) {
    case CwbvhShape::kVariant90:   // diagnostic: the incoherent flavor whatever the batch (tests, tools/ab_configs.py)
        launch_cwbvh(L.any, 0, s->cw.hybrid, s->cw.trisPadded, q, c->status, P.blocksBase, L.st, 13, P.small, P.blocks7Cwbvh);
        break;
    case CwbvhShape::kVariant91: {   // diagnostic: the coherent flavor (deferred triangles, gated triangle phase) whatever the batch and its probe say
        QueryArgs qa = q;
        qa.probe = L.probeLine; qa.baseBlocks = 0; qa.flags |= 16u;
        launch_cwbvh(L.any, 0, s->nodes, tris, qa, c->status, P.blocks, L.st, 5, P.small, P.blocks7Cwbvh);
        break;
    }
    case CwbvhShape::kVariant92:   // diagnostic: one traversal per wave of 64 consecutive rays (kernels_cwbvh_packet.hip) whatever batch, scene and tuner
        launch_cwbvh_packet(L.any, s->nodes, s->tris, q, c->status, P.blocks, L.st);
        break;
    case CwbvhShape::kTwoFlavors:
    case CwbvhShape::kFlavorAndBehind:
        // Solo (only ever a kTwoFlavors launch: launch_plan.h, soloCandidate): the coherent flavor is left out.  The prediction decides nothing about which
        // rays are traced: the incoherent flavor never looks at a verdict and draws every ray from the pool (as under variant 90), so a batch that has turned
        // coherent is traced correctly, once, by the slower flavor; its block 0 publishes the sample, the host sees the coherent vote when the launch has
        // finished, and the buffer's next launch is two flavors again.  What is saved is a kernel of 8192 workgroups that sample and leave — 16 us into an
        // idle GPU, but a stream barrier in front of the real kernel when the launch starts beside another lane's persistent waves (every slot taken: the
        // dead flavor's last workgroup runs when that kernel retires).
        if (L.solo) {   // (what launchCoherentFlavor keeps for tbvh_debug_coherent_schedule is kept too: the latest launch's class, the launches counted)
            q.flags |= 64u; c->soloLaunches++;
            s->cohLastClass[L.any ? 1 : 0] = (uint8_t)P.sizeClass;
            s->cohTuner[L.any ? 1 : 0][P.sizeClass].launches++;
        } else if (int r = launchCoherentFlavor(s, q, P, L, tris)) return r;
        if (P.shape == CwbvhShape::kFlavorAndBehind) {   // behind it: the scene's unprobed kernel, as launched without a probe
            QueryArgs qp = q;
            qp.probe = nullptr; qp.baseBlocks = 0;
            launchSceneKernel(s, qp, P, L, tris);
        } else {
            // the incoherent flavor on 28 one-wave workgroups per CU when the batch fills the grid (24 is the persistent grid's size: 20 / 26 / 28 / 30 /
            // 32 per CU trace bounce rays at -4.4 / +0.6 / +0.9 / +0.5 / +0.5 %, interleaved medians of 13 rounds)
            uint32_t wX = (c->expFlags >> 8) & 0xffu;   // experiment: another number of waves per CU
            if (wX > 32u) wX = 32u;                     // (the spill area holds blocks + blocks / 3 = 32 workgroups per CU: LaneStack strides by gridDim)
            const uint32_t wB = wX ? wX : (c->gridOverride ? 0u : 28u);
            const uint32_t blocksIncoherent = (wB && P.blocksBase == c->blocks) ? (uint32_t)c->numCUs * wB : P.blocksBase;
            launch_cwbvh(L.any, 0, s->cw.hybrid, s->cw.trisPadded, q, c->status, blocksIncoherent, L.st, 13, P.small, P.blocks7Cwbvh);
        }
        break;
    case CwbvhShape::kOneKernel:
        launchSceneKernel(s, q, P, L, tris);
        break;
    }
    return 0;
}

// Lane 1 of the context with what a launch on it needs (its stream, counter areas and stack spill area), made by the first launch that would take
// it.  false: it cannot be had (no memory): launches do not overlap on this context, which is never an error of the query.
static bool ensureLane1(tbvh_context* c) {
    tbvh_context::Lane1& l = c->lane1;
    if (l.unusable) return false;
    if (l.stream && l.pool && l.spill && c->evBase) return true;
    const size_t spillWords = (size_t)(c->blocks + c->blocks / 3u) * 64 * c->spillEntries;   // (as lane 0's: the largest grid any launch uses)
    if ((!c->evBase && hipEventCreateWithFlags(&c->evBase, hipEventDisableTiming) != hipSuccess) ||
        (!l.stream && hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking) != hipSuccess) ||
        (!l.pool && l.pool.alloc(kPoolWords * 2) != hipSuccess) || (!l.spill && l.spill.alloc(spillWords) != hipSuccess)) {
        (void)hipGetLastError();
        l.pool.reset(); l.spill.reset();
        l.unusable = true;
        return false;
    }
    l.poolClean = false;
    return true;
}

// The host's side of the probe's verdicts (probe_memory.h): two words per entry of the event ring in host-coherent pinned memory, made by the first probed
// launch.  Block 0 of the kernel that publishes a launch's probe counts stores them there as well (cwbvh_probe.h: probe_publish) — no copy goes into the
// stream — and the host reads a launch's words only after it has seen that launch's end event complete.  false: no such memory (every launch two flavors).
static bool ensureProbeSlots(tbvh_context* c) {
    if (c->probeSlots) return true;
    if (c->probeSlotsFailed) return false;
    void* p = nullptr;
    if (hipHostMalloc(&p, (size_t)tbvh_context::kTimeRing * 2 * sizeof(uint32_t), hipHostMallocCoherent) != hipSuccess || !p) {
        (void)hipGetLastError();
        c->probeSlotsFailed = true;
        return false;
    }
    memset(p, 0, (size_t)tbvh_context::kTimeRing * 2 * sizeof(uint32_t));
    c->probeSlots = (uint32_t*)p;
    return true;
}

// ---- has a launch finished? ---------------------------------------------------------------------------------------------------------------------
// One question to the runtime, never a wait: the end event of the launch whose event pair is entry `slot` of the ring.
enum EndState { kInFlight = 0, kEnded = 1, kCannotTell = 2 };   // kCannotTell: the query itself failed
static EndState endEventState(tbvh_context* c, uint32_t slot) {
    const hipError_t qe = hipEventQuery(c->evRing[slot][1]);
    if (qe == hipSuccess) return kEnded;
    (void)hipGetLastError();
    return qe == hipErrorNotReady ? kInFlight : kCannotTell;
}
// Its three readers differ in how they name a launch and in what they make of one the ring no longer holds (its event pair has gone to a later operation):
// LaneBook::prune names a record by its slot: whatever is not in flight leaves the list;
static bool recordHasLeft(tbvh_context* c, uint32_t slot) { return endEventState(c, slot) != kInFlight; }
// LaneBook::gate names a launch by its number: one the ring no longer holds is kTimeRing operations back and counts as finished, never waited for;
static bool finishedOrForgotten(tbvh_context* c, uint64_t seq) {
    return !c->ringHolds(seq) || endEventState(c, (uint32_t)(seq % tbvh_context::kTimeRing)) != kInFlight;
}
// ProbeMemory::harvest likewise by number: such a launch (or any, without the verdict slots) leaves without a vote — kCannotTell; kEnded: its words are read.
static EndState verdictState(tbvh_context* c, uint64_t seq) {
    if (!c->ringHolds(seq) || !c->probeSlots) return kCannotTell;
    return endEventState(c, (uint32_t)(seq % tbvh_context::kTimeRing));
}

// Verdicts of the remembered launches that have finished by now join the table.  Never waits: a launch still in flight stays remembered, one whose event
// pair the ring has handed to a later operation leaves without a vote.
static void harvestVerdicts(tbvh_context* c) {
    c->probeMemory.harvest(
        [c](uint64_t seq) { return (int)verdictState(c, seq); },
        [c](uint64_t seq) {
            const volatile uint32_t* w = c->probeSlots + 2 * (seq % tbvh_context::kTimeRing);
            const uint32_t agree = w[0], pairs = w[1];
            if (!pairs) return (int)ProbeMemory::kNone;
            c->probeVerdicts++;
            return (int)(agree * 10u >= pairs * 6u ? ProbeMemory::kCoherent : ProbeMemory::kIncoherent);   // the rule of k_cwbvh (kernels_cwbvh.hip)
        });
}

// Something the launch does before its kernels would enqueue work on lane 0 or replace arrays that launches in flight read (a derived copy made or made
// again, a TLAS re-classified): such a launch joins the lanes first.
static bool launchPrepares(const tbvh_scene* s, uint64_t n, bool any) {
    if (s->isTlas) return s->tlas.blasRecopyPending || (any && !s->tlas.anyHitSeen && !s->tlas.blasSpheres);
    if (s->copies.pending()) return true;
    if (s->triTest && !s->copies.copy8 && (s->layout == TBVH_LAYOUT_BVH_GPU || s->layout == TBVH_LAYOUT_BVH4_GPU)) return true;   // (ensureWatertightCopy)
    return n >= 1024u && s->variant == 0 && !s->copies.tried8 && (s->layout == TBVH_LAYOUT_BVH_GPU || s->layout == TBVH_LAYOUT_BVH4_GPU);
}

// ---- launchQuery's steps, in the order it takes them ---------------------------------------------------------------------------------------------------
// Step 1, the scene: what a query does to it before anything is launched (none of it part of the query's time).  *wide: the scene the query runs on
// instead — a BVH_GPU / BVH4_GPU scene with an 8-wide copy (capi_copies.hip) —, for which the caller starts over.
static int prepareScene(tbvh_scene* s, uint64_t n, bool any, bool sizeKnown, tbvh_scene** wide) {
    s->raysTraced += n;   // (what tbvh_refit weighs the refit of a scene's copies against)
    countQueryForRecopy(s);   // copies dropped by a tbvh_update_* come back once the blob has settled
    if (!s->isTlas && (!sizeKnown || n >= 1024u)) makeCopyOnce(s, kCopyWide8);   // first query of a BVH_GPU / BVH4_GPU scene
    if (s->triTest && !s->isTlas) if (int r = ensureWatertightCopy(s)) return r;   // a watertight BVH_GPU / BVH4_GPU scene: the 8-wide copy whatever the batch
    if ((*wide = wideCopyForQuery(s))) return 0;
    // the first IsOccluded through this TLAS: its BVH4_GPU and BVH_GPU BLASes are entered through 8-wide copies by any-hit queries
    if (any && s->isTlas && !s->tlas.anyHitSeen && !s->tlas.blasSpheres) {
        s->tlas.anyHitSeen = true;
        for (tbvh_scene* b : s->tlas.blasList) makeCopyOnce(b, kCopyWide8);   // (re-classifies the TLASes over b, this one included)
        if (int r = reclassifyTlas(s)) return r;
    }
    return 0;
}

static QueryArgs queryArgsOf(const tbvh_scene* s, RayRec* d_rays, uint64_t n, uint8_t* d_occ, bool fresh, float freshTmax, const unsigned long long* nDev) {
    const tbvh_context* c = s->ctx;
    QueryArgs q;   // (stats and hybridK share their storage with a watertight scene's wtVerts and wtTris — device_common.h —, which only launchCwbvhKernels sets, on
                   // the copy it hands its watertight kernels: whoever else builds a QueryArgs for such a scene must set them too)
    q.rays = d_rays; q.nRays = n; q.occluded = d_occ;
    q.poolParts = c->poolParts;
    q.stats = c->counter + 8;
    q.fresh = fresh ? 1u : 0u; q.freshTmax = freshTmax; q.nRaysDev = nDev; q.omm = Omm{s->opmap, s->opmapN};
    q.probe = nullptr; q.baseBlocks = 0; q.hybridK = s->cw.packed; q.flags = 0u;
#ifdef TBVH_EXPERIMENTS
    q.flags = c->expFlags & 0x3FF0001u;
#endif
    q.splitBelow = c->splitBelow;
    return q;
}

// Step 2, the plan (launch_plan.h): the facts of this launch, planBatch, what `probed` asks of the scene, planShape over the copies as they then are.
static int planLaunch(tbvh_scene* s, uint64_t n, bool sizeKnown, const Launch& L, LaunchPlan* plan) {
    tbvh_context* c = s->ctx;
    LaunchFacts f;
    f.isTlas = s->isTlas; f.layout = s->layout; f.variant = s->variant; f.n = n; f.sizeKnown = sizeKnown; f.any = L.any;
    f.blobBytes = (!s->isTlas && s->layout == TBVH_LAYOUT_CWBVH) ? (s->nNodeBlocks + s->nTriBlocks) * 16 : sceneBytes(s);   // (BVH8_CWBVH: without the library's own copies)
    f.gridOverride = c->gridOverride; f.numCUs = (uint32_t)c->numCUs; f.blocks = c->blocks; f.raysPerBlock = c->raysPerBlock;
    f.expFlags = c->expFlags; f.cohTunerMode = c->cohTunerMode; f.probeMemoryOn = c->probeMemoryOn; f.skipTiming = c->skipTiming;
    f.triTest = s->triTest;
    for (int k = 0; k < 4; k++) f.decided[k] = s->cohTuner[L.any ? 1 : 0][k].decided;
    *plan = planBatch(f);
    if (plan->probed && !s->cw.tried) {   // first launch of this class on the scene: the derived copies for incoherent batches (not part of the query's time)
        if (L.overlaps) if (int r = joinLanes(c)) return r;   // (built on lane 0)
        if (int r = prepareIncoherentCopies(s)) return r;
    }
    f.hasPadded = s->cw.padded != nullptr; f.hasHybrid = s->cw.hybrid != nullptr; f.hasTrisPadded = s->cw.trisPadded != nullptr;
    planShape(*plan, f);
    if (plan->probedSmallCancelled) s->cohLastClass[L.any ? 1 : 0] = (uint8_t)plan->sizeClass;
    return 0;
}

// Step 3, the lane of a launch that may overlap others (L.overlaps).
// A launch the scene's CohTuner may time (a two-flavor launch of a class still undecided) and the launch after it run serialised: a sample taken
// beside another launch's tail must not decide a schedule.
static int chooseLane(tbvh_context* c, bool tunerMeasures, Launch& L) {
    // (lane 1 is made by the first launch that MAY overlap, also one that does not: its stack spill area is a large allocation — 10 ms on the bench's
    // context —, which belongs to a caller's warm-up launches, serialised by the tuner or not, and not to the first launch that finds a neighbour in flight)
    const bool haveLane1 = ensureLane1(c);
    if (tunerMeasures || c->serialiseNext) {
        if (int r = joinLanes(c)) return r;
        c->serialiseNext = tunerMeasures;
        return 0;
    }
    c->book.prune([c](int, uint32_t slot) { return recordHasLeft(c, slot); });
    const LaneChoice ch = c->book.decide(L.fp, haveLane1);
    if (ch.join) { if (int r = joinLanes(c)) return r; }
    L.lane = ch.lane;
    // What was enqueued on lane 0 before its in-flight query launches (ray generators, uploads, refits) comes before a launch on lane 1 too: evBase marks
    // that position — NOT lane 0's end, which would put the launch behind the very launches it may overlap.
    if (c->lane0Touched && c->evBase) {
        HIP_TRY(hipEventRecord(c->evBase, c->stream));
        c->lane0Touched = false; c->lane1SawBase = false;
    }
    if (L.lane == 1 && !c->lane1SawBase) {
        HIP_TRY(hipStreamWaitEvent(c->lane1.stream, c->evBase, 0));
        c->lane1SawBase = true;
    }
    // Launches START in the order they were enqueued, across the lanes too, give or take overlapDepth launches (LaneBook::gate): this one waits for the
    // start (not the end) of one of the other lane's last launches.  Depth 1, the latest: neither lane runs more than one launch ahead of the other.
    // Depth 2, the one before the latest, while it is in flight: a caller alternating camera and bounce batches (C1 D1 C2 D2 ...) gets C(k+2) into the
    // tail of D(k) — at depth 1 it waits for the start of D(k+1), which stream order holds behind D(k)'s end, and lane 0 sits empty for exactly that
    // tail.  The camera launch still takes the wave slots first: it starts in D(k)'s tail, D(k+1) behind D(k)'s end.  Either way the launches that ran
    // beside a launch are its near neighbours in the order enqueued (what timedMs looks at).  Measured (profiles/r09_runahead.txt): depth 2 alone +1.3 %
    // on the bench step.  That C(k+2) meets D(k) at all is the dead coherent flavor's doing: in front of D(1) it cannot finish before C(1) retires, so
    // D(1) starts at C(1)'s end and every D(k) runs beside C(k+1).  Launched as one kernel (the probe memory, armProbe) D(k) starts beside C(k), C(k+1) waits
    // for a start long past and takes D(k)'s tail at depth 1 already: depth 2 adds nothing then, so the default is 1.
    // (A start event the ring has given to a later operation stands for a launch kTimeRing operations back: finishedOrForgotten.)
    const uint64_t g = c->book.gate(L.lane, c->overlapDepth, [c](uint64_t seq) { return finishedOrForgotten(c, seq); });
    if (g != LaneBook::kNoGate && c->ringHolds(g))
        HIP_TRY(hipStreamWaitEvent(L.lane ? c->lane1.stream : c->stream, c->evRing[g % tbvh_context::kTimeRing][0], 0));
    return 0;
}

// Step 4, the lane's counter pool and spill area.
// ray-fetch counters: two areas alternate; the kernels of this launch zero the other area for the next one ON THE SAME LANE (each lane has its own
// pair: a launch overlapping this one would otherwise draw from the area this one is zeroing).  After anything that went wrong between two launches
// (poolClean still false) both are cleared here.
static int bindLanePool(tbvh_context* c, Launch& L, QueryArgs& q) {
    uint32_t* const pool = L.lane ? c->lane1.pool.get() : c->pool.get();
    const int poolCur = L.lane ? c->lane1.poolCur : c->poolCur;
    bool& poolClean = L.lane ? c->lane1.poolClean : c->poolClean;
    if (!poolClean) HIP_TRY(hipMemsetAsync(pool, 0, kPoolWords * 4 * 2, L.st));
    poolClean = false;
    q.spill = L.lane ? c->lane1.spill : c->spill; q.counter = pool + (size_t)poolCur * kPoolWords; q.counterNext = pool + (size_t)(poolCur ^ 1) * kPoolWords;
    L.probeLine = q.counter + (size_t)kPoolParts * kPoolCounterStride;
    return 0;
}

// Step 6, the probe: its counters for a probed launch, and what the probe said about this buffer's last launches (probe_memory.h).  A probed launch whose
// size the host knows gets a slot for its verdict (the slot of its event pair) and is remembered until it is seen finished.  It goes SOLO — the incoherent
// flavor alone, launchCwbvhKernels — when the last two finished launches with exactly this footprint both voted incoherent, the scene's tuner has settled
// this class of batch (it must see every coherent launch it would have seen) and nothing diagnostic is set (launch_plan.h: soloCandidate, wantsVerdictSlot).
// Any doubt: two flavors, as without the memory.
static void armProbe(tbvh_scene* s, const LaunchPlan& plan, Launch& L, QueryArgs& q) {
    tbvh_context* c = s->ctx;
    if (plan.probed || plan.probedSmall) {
        q.probe = L.probeLine; q.baseBlocks = plan.blocksBase;
        c->lastProbed = true; c->lastProbedLane = L.lane;
    }
    if (c->probeMemory.nPending) harvestVerdicts(c);
    if (plan.wantsVerdictSlot && ensureProbeSlots(c)) {
        L.key.lo = L.fp.rays.lo; L.key.hi = L.fp.rays.hi; L.key.scene = s; L.key.any = L.any; L.remember = true;
        uint32_t* const slot = c->probeSlots + 2 * (size_t)L.ringSlot;
        slot[0] = slot[1] = 0u;   // (pairs == 0: no verdict)
        q.probeHost = slot;
        L.solo = s->cohTuner[L.any ? 1 : 0][plan.sizeClass].decided != 0 && c->probeMemory.solo(L.key);
    }
}

// Step 7, the kernels, by the scene's kernel family.
static int enqueueKernels(tbvh_scene* s, QueryArgs& q, const LaunchPlan& plan, const Launch& L) {
    tbvh_context* c = s->ctx;
    const KernelFamily family = kernelFamily(s, L.any);
    const TlasKindPlan t = s->isTlas ? tlasKind(s, L.any) : TlasKindPlan();
    const BlasDesc* const desc = s->isTlas ? tlasDesc(s, L.any) : nullptr;
    const uint32_t blocks = plan.blocks, blocks7 = plan.blocks7Tlas;
    q.spillStride = stackEntriesPerLane(s, L.any, family);
    if (s->isTlas && s->tlas.plan.watertight && family != KernelFamily::kTlas8)   // (a missing kernel is an error, never another kernel)
        return fail(TBVH_E_INVALID, "a TLAS over watertight BLASes without its 8-wide tree: no other two-level kernel has a watertight form");
    switch (family) {
    case KernelFamily::kBvh2: launch_bvh2(L.any, s->variant, s->nodes, s->tris, q, c->status, blocks, L.st); break;
    case KernelFamily::kBvh4: launch_bvh4(L.any, s->variant, s->nodes, q, c->status, blocks, L.st); break;
    case KernelFamily::kCwbvh: return launchCwbvhKernels(s, q, plan, L);
    case KernelFamily::kSphere: launch_custom(L.any, s->nodes, s->tris, q, c->status, blocks, L.st); break;
    case KernelFamily::kVoxel: launch_voxel(L.any, (const uint32_t*)s->nodes.get(), nullptr, nullptr, nullptr, nullptr, q, c->status, blocks, L.st); break;
    case KernelFamily::kTlasSphere: launch_tlas_custom(L.any, t.layout, s->nodes, s->tlas.tlasIdx, s->tlas.instances, desc, q, c->status, blocks, L.st); break;
    case KernelFamily::kTlas4: launch_tlas4(L.any, 0, s->tlas.tlas4, s->tlas.instances, desc, q, c->status, blocks, L.st, blocks7); break;
    case KernelFamily::kTlas8: launch_tlas8(L.any, 0, s->tlas.tlas8, s->tlas.tlas8Refs, s->tlas.instances, desc, q, c->status, blocks, L.st, blocks7, t.mix, s->tlas.plan.watertight); break;
    case KernelFamily::kTlasVoxel: launch_voxel(L.any, nullptr, s->nodes, s->tlas.tlasIdx, s->tlas.instances, desc, q, c->status, blocks, L.st); break;
    case KernelFamily::kTlas2: launch_tlas2(L.any, 0, s->nodes, s->tlas.tlasIdx, s->tlas.instances, desc, q, c->status, blocks, L.st, blocks7); break;
    case KernelFamily::kTlasFlat: launch_tlas(L.any, t.layout, s->nodes, s->tlas.tlasIdx, s->tlas.instances, desc, q, c->status, blocks, L.st); break;
    case KernelFamily::kNone: return fail(TBVH_E_INVALID, "scene layout %d has no query kernel", s->layout);
    }
    return 0;
}

// Step 8, the launch's end, once its kernels are enqueued: the end event, the lane's record of it, the other counter area now zeroed by what was enqueued.
static int finishLaunch(tbvh_context* c, const Launch& L) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c, L.st));
    (L.lane ? c->lane1.poolCur : c->poolCur) ^= 1; (L.lane ? c->lane1.poolClean : c->poolClean) = true;
    if (L.overlaps) {
        c->book.add(L.lane, L.fp, L.ringSlot, L.launchSeq);
        c->evChain[L.ringSlot] = c->chain;
        if (L.lane) { c->lane1Last = c->evRing[L.ringSlot][1]; c->lane1Dirty = true; c->lane1Launches++; }
    }
    if (L.remember) c->probeMemory.note(L.key, L.launchSeq, L.lane);
    return 0;
}

int launchQuery(tbvh_scene* s, RayRec* d_rays, uint64_t n, uint8_t* d_occ, bool fresh, float freshTmax, const unsigned long long* nDev, bool mayOverlap) {
    tbvh_context* c = s->ctx;
    TBVH_LOCK(c);
    Launch L;
    L.any = d_occ != nullptr;
    // Two lanes (overlap_lanes.h): a device-resident query whose buffers no launch in flight touches need not wait for the launches before it — the
    // persistent grids fill every wave slot, so its workgroups start where the earlier launch's waves retire and its body hides that launch's tail.
    // Everything else (and every launch while overlap is off, on a caller's stream, untimed or sized on the device) joins the lanes like any entry point.
    L.overlaps = mayOverlap && c->overlap && c->stream == c->ownStream && !c->skipTiming && !nDev && n != 0 && !launchPrepares(s, n, L.any);
    if (L.overlaps) HIP_TRY(hipSetDevice(c->device));
    else if (int r = setDevice(c)) return r;
    if (n == 0) return 0;
    tbvh_scene* wide = nullptr;
    if (int r = prepareScene(s, n, L.any, nDev == nullptr, &wide)) return r;
    if (wide) return launchQuery(wide, d_rays, n, d_occ, fresh, freshTmax, nDev, mayOverlap);
    L.fp = footprintOf(d_rays, n, d_occ);
    QueryArgs q = queryArgsOf(s, d_rays, n, d_occ, fresh, freshTmax, nDev);
    c->lastProbed = false;
    LaunchPlan plan;
    if (int r = planLaunch(s, n, nDev == nullptr, L, &plan)) return r;
    q.hybridK = s->cw.packed;   // (as the copies now are)
    if (L.overlaps) if (int r = chooseLane(c, plan.tunerMeasures, L)) return r;
    L.st = L.lane ? c->lane1.stream : c->stream;
    if (int r = bindLanePool(c, L, q)) return r;
    HIP_TRY(timedBegin(c, L.st));   // step 5
    L.launchSeq = c->evSeq - 1; L.ringSlot = (uint32_t)(L.launchSeq % tbvh_context::kTimeRing);   // (lanes, probe memory: timing is on, it has its event pair)
    armProbe(s, plan, L, q);
    if (int r = enqueueKernels(s, q, plan, L)) return r;
    return finishLaunch(c, L);
}

int checkStatus(tbvh_context* c) {
    static const struct { uint32_t bit; const char* message; } kStatusErrors[] = {   // in the order they are looked for: the first bit found is reported
        {1u, "traversal stack overflow (tree deeper than the spill area allows)"},
        {2u, "refit: a triangle record refers to a primitive beyond the vertex array"},
        {4u, "wide TLAS build: the node capacity did not hold the collapsed tree"},
        {16u, "sphere query: a triangle record refers to a primitive beyond the vertex array"},
        {kStatusMeshIndex, "mesh: a vertex index of a device-resident index buffer is not a vertex (index >= n_verts)"},
        {kStatusPoseJoint, "pose: a joint index of a device-resident joint array is not a joint (index >= n_joints); that vertex was not written"},
        {kStatusOmmIndex, "opacity micromap bake: a device-resident index is not a UV (>= n_uv; clamped) or a texture index is not a texture (>= n_textures; "
                          "taken as none)"},
        {kStatusGraph, "scene graph: a sampler, node, key state or key position of a graph was out of range on the device; that channel, node, instance or "
                       "joint was not written"},
        {kStatusShade, "shade: a hit record's instance, BLAS slot or primitive, or a device-resident material or texture index, is out of range (the record "
                       "got no surface, or an untextured albedo of 0)"},
        {kStatusWatertightPrim, "watertight test: a triangle record names a primitive beyond the vertices given to tbvh_set_triangle_test (that triangle was no hit)"},
        {kStatusVoxelNormal, "voxel normals: a hit record's instance index is not an instance of the TLAS (that record got zeros)"},
    };
    uint32_t st = 0;
    if (int r = joinLanes(c)) return r;   // (launches on lane 1 set the status word too)
    HIP_TRY(hipMemcpyAsync(&st, c->status, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const auto& e : kStatusErrors)
        if (st & e.bit) {
            hipMemsetAsync(c->status, 0, 4, c->stream);
            return fail(TBVH_E_FORMAT, "%s", e.message);
        }
    return 0;
}
}  // namespace tbvh_capi

extern "C" {

// ---- queries ---------------------------------------------------------------------------

int tbvh_intersect_device(tbvh_scene* s, void* dRays, uint64_t n) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_intersect_device");
    if (!s || (!dRays && n)) return fail(TBVH_E_INVALID, "tbvh_intersect_device: null argument");
    if (((uintptr_t)dRays) & 15) return fail(TBVH_E_INVALID, "ray array must be 16-byte aligned");
    return launchQuery(s, (RayRec*)dRays, n, nullptr, false, 1e30f, nullptr, true);
}

int tbvh_intersect_device_fresh(tbvh_scene* s, void* dRays, uint64_t n, float tmax) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_intersect_device_fresh");
    if (!s || (!dRays && n)) return fail(TBVH_E_INVALID, "tbvh_intersect_device_fresh: null argument");
    if (((uintptr_t)dRays) & 15) return fail(TBVH_E_INVALID, "ray array must be 16-byte aligned");
    return launchQuery(s, (RayRec*)dRays, n, nullptr, true, tmax, nullptr, true);
}

int tbvh_occluded_device(tbvh_scene* s, const void* dRays, uint64_t n, uint8_t* dOcc) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_occluded_device");
    if (!s || ((!dRays || !dOcc) && n)) return fail(TBVH_E_INVALID, "tbvh_occluded_device: null argument");
    if (((uintptr_t)dRays) & 15) return fail(TBVH_E_INVALID, "ray array must be 16-byte aligned");
    return launchQuery(s, (RayRec*)dRays, n, dOcc, false, 1e30f, nullptr, true);
}

int tbvh_intersect(tbvh_scene* s, void* rays, uint64_t n, uint32_t stride) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_intersect");
    if (!s || (!rays && n)) return fail(TBVH_E_INVALID, "tbvh_intersect: null argument");
    if (stride < 64 || (stride & 3)) return fail(TBVH_E_INVALID, "stride must be >= 64 and a multiple of 4 (got %u)", stride);
    if (n == 0) return 0;
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    return hostQuery(s, (const char*)rays, (char*)rays, n, stride, nullptr);   // pinned, chunked, multi-threaded, pipelined staging (capi_query.hip: hostQuery)
}

int tbvh_occluded(tbvh_scene* s, const void* rays, uint64_t n, uint32_t stride, uint8_t* occ) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_occluded");
    if (!s || ((!rays || !occ) && n)) return fail(TBVH_E_INVALID, "tbvh_occluded: null argument");
    if (stride < 64 || (stride & 3)) return fail(TBVH_E_INVALID, "stride must be >= 64 and a multiple of 4 (got %u)", stride);
    if (n == 0) return 0;
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    return hostQuery(s, (const char*)rays, nullptr, n, stride, occ);
}

// ---- page-locked host memory FROM the library: the tinyocl::Buffer( bytes ) of this boundary (tiny_ocl.h: a Buffer made without a host pointer owns
// ---- its host side; tiny_bvh_speedtest.cpp:1101-1108 wraps its ray array in one before every GPU block) -----------------------------------------
// Round 5 first page-locked the CALLER's memory (hipHostRegister): with that in the process, later plain hipMemcpy calls from pageable memory that
// had been registered, unregistered, freed and handed out again by the allocator faulted the GPU ("Memory access fault ... Reason: Unknown", 3 runs of the
// GPU suite in 9; 0 in 6 without the registering tests).  The library therefore never registers foreign memory: it hands out memory of its own.
int tbvh_pinned_malloc(tbvh_context* c, uint64_t bytes, void** out) {
    if (!c || !out || !bytes) return fail(TBVH_E_INVALID, "tbvh_pinned_malloc: null/empty argument");
    TBVH_ENTER(c);
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess || !p) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "tbvh_pinned_malloc: cannot page-lock %llu bytes", (unsigned long long)bytes); }
    try { c->pinned.push_back(tbvh_context::PinnedRange{(char*)p, bytes}); }
    catch (const std::bad_alloc&) { hipHostFree(p); return fail(TBVH_E_NOMEM, "out of host memory"); }
    *out = p;
    return 0;
}

int tbvh_pinned_free(tbvh_context* c, void* ptr) {
    if (!c || !ptr) return fail(TBVH_E_INVALID, "tbvh_pinned_free: null argument");
    TBVH_ENTER(c);
    for (size_t i = 0; i < c->pinned.size(); i++)
        if (c->pinned[i].host == (char*)ptr) {
            HIP_TRY(hipStreamSynchronize(c->stream));   // nothing of this context may still be reading the range
            c->pinned.erase(c->pinned.begin() + i);
            HIP_TRY(hipHostFree(ptr));
            return 0;
        }
    return fail(TBVH_E_INVALID, "tbvh_pinned_free: %p did not come from tbvh_pinned_malloc of this context", ptr);
}

// ---- one ray array over several devices -----------------------------------------------------------
// The BVH is replicated (scenes[i] = the same blobs uploaded through context i), the ray array is cut into contiguous,
// wave-aligned shards (the same arithmetic as tinybvh_amd/sharding.py: shard_range), one host thread per device drives
// that device's staging + kernel + read-back, results land in the caller's array in place.  No collective.
void tbvh_shard_range(uint64_t n_rays, uint32_t rank, uint32_t world, uint64_t* begin, uint64_t* end) {
    const uint64_t align = 64, units = (n_rays + align - 1) / align;
    const uint64_t base = world ? units / world : 0, extra = world ? units % world : 0;
    const uint64_t b = (uint64_t)rank * base + (rank < extra ? rank : extra), e = b + base + (rank < extra ? 1 : 0);
    if (begin) *begin = b * align < n_rays ? b * align : n_rays;
    if (end) *end = e * align < n_rays ? e * align : n_rays;
}

namespace {
int shardedQuery(tbvh_scene* const* scenes, uint32_t nDev, void* rays, uint64_t n, uint32_t stride, uint8_t* occ, const char* who) {
    if (!scenes || nDev == 0 || (!rays && n)) return fail(TBVH_E_INVALID, "%s: null/empty argument", who);
    if (stride < 64 || (stride & 3)) return fail(TBVH_E_INVALID, "stride must be >= 64 and a multiple of 4 (got %u)", stride);
    for (uint32_t i = 0; i < nDev; i++) {
        if (!scenes[i]) return fail(TBVH_E_INVALID, "%s: scene %u is null", who, i);
        TBVH_REFUSE_DOUBLE(scenes[i], who);
        if (scenes[i]->layout != scenes[0]->layout || scenes[i]->isTlas != scenes[0]->isTlas) return fail(TBVH_E_INVALID, "%s: scene %u is not a replica of scene 0 (layout differs)", who, i);
        for (uint32_t j = 0; j < i; j++) if (scenes[j]->ctx == scenes[i]->ctx) return fail(TBVH_E_INVALID, "%s: scenes %u and %u share a context (one context, i.e. one stream and staging area, per shard)", who, j, i);
    }
    if (n == 0) return 0;
    std::vector<int> rc(nDev, 0);
    std::vector<std::string> msg(nDev);
    auto work = [&](uint32_t i) {
        uint64_t b, e;
        tbvh_shard_range(n, i, nDev, &b, &e);
        if (e == b) return;
        char* base = (char*)rays + b * stride;
        rc[i] = occ ? tbvh_occluded(scenes[i], base, e - b, stride, occ + b) : tbvh_intersect(scenes[i], base, e - b, stride);
        if (rc[i]) msg[i] = tbvh_last_error();   // the worker's thread-local message
    };
    std::vector<std::thread> th;
    for (uint32_t i = 1; i < nDev; i++) th.emplace_back(work, i);
    work(0);
    for (auto& t : th) t.join();
    for (uint32_t i = 0; i < nDev; i++) if (rc[i]) return fail(rc[i], "%s: shard %u (device %d): %s", who, i, scenes[i]->ctx->device, msg[i].c_str());
    return 0;
}
}  // namespace

int tbvh_intersect_sharded(tbvh_scene* const* scenes, uint32_t nDev, void* rays, uint64_t n, uint32_t stride) {
    return shardedQuery(scenes, nDev, rays, n, stride, nullptr, "tbvh_intersect_sharded");
}
int tbvh_occluded_sharded(tbvh_scene* const* scenes, uint32_t nDev, const void* rays, uint64_t n, uint32_t stride, uint8_t* occ) {
    if (!occ && n) return fail(TBVH_E_INVALID, "tbvh_occluded_sharded: null output");
    return shardedQuery(scenes, nDev, (void*)rays, n, stride, occ, "tbvh_occluded_sharded");
}

// ---- device-resident rays over several devices: nothing crosses the host -------------------------------------------------------------
// Every device's launch is asynchronous on its context's stream, so ONE host thread enqueues them all (a few tens of microseconds each:
// dispatch_ms[i] = host time spent enqueueing device i's launch), then waits for all.  With the rays produced and consumed where they are
// traced — a wavefront path tracer per device (tbvh_wavefront_render_sharded), or rays a kernel of the caller's wrote — the devices run
// at their device-resident rate; tbvh_intersect_sharded above moves HOST rays and is bound by the host (DESIGN.md par. 7).
namespace {
int shardedDeviceQuery(tbvh_scene* const* scenes, uint32_t nDev, void* const* dRays, const uint64_t* nRays, uint8_t* const* dOcc, int fresh, float tmax,
                       float* kernelMs, float* dispatchMs, const char* who) {
    if (!scenes || !nDev || !dRays || !nRays) return fail(TBVH_E_INVALID, "%s: null argument", who);
    for (uint32_t i = 0; i < nDev; i++) {
        if (!scenes[i]) return fail(TBVH_E_INVALID, "%s: scenes[%u] is null", who, i);
        TBVH_REFUSE_DOUBLE(scenes[i], who);
        if (nRays[i] && (!dRays[i] || (dOcc && !dOcc[i]))) return fail(TBVH_E_INVALID, "%s: null ray / output pointer for device %u", who, i);
        for (uint32_t k = 0; k < i; k++) if (scenes[k]->ctx == scenes[i]->ctx) return fail(TBVH_E_INVALID, "%s: scenes %u and %u share a context (one scene per context)", who, k, i);
    }
    int rc = 0;
    uint32_t launched = 0;
    for (; launched < nDev && !rc; launched++) {
        const uint32_t i = launched;
        const auto t0 = std::chrono::steady_clock::now();
        rc = launchQuery(scenes[i], (RayRec*)dRays[i], nRays[i], dOcc ? dOcc[i] : nullptr, fresh != 0, tmax);
        if (dispatchMs) dispatchMs[i] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // wait for everything that was enqueued, also after a failure: the caller gets its buffers back quiescent (the first error is reported)
    std::string firstErr = rc ? tbvh_last_error() : "";
    for (uint32_t i = 0; i < launched; i++) {
        if (!nRays[i]) { if (kernelMs) kernelMs[i] = 0.f; continue; }
        const int r = checkStatus(scenes[i]->ctx);   // synchronizes device i's stream
        if (r && !rc) { rc = r; firstErr = tbvh_last_error(); }
        if (kernelMs) kernelMs[i] = r ? -1.f : tbvh_time_last_ms(scenes[i]->ctx);
    }
    if (rc) return fail(rc, "%s: %s", who, firstErr.c_str());
    return 0;
}
}  // namespace

int tbvh_intersect_sharded_device(tbvh_scene* const* scenes, uint32_t nDev, void* const* dRays, const uint64_t* nRays, int fresh, float tmax,
                                  float* kernelMs, float* dispatchMs) {
    return shardedDeviceQuery(scenes, nDev, dRays, nRays, nullptr, fresh, tmax, kernelMs, dispatchMs, "tbvh_intersect_sharded_device");
}
int tbvh_occluded_sharded_device(tbvh_scene* const* scenes, uint32_t nDev, const void* const* dRays, const uint64_t* nRays, uint8_t* const* dOcc,
                                 float* kernelMs, float* dispatchMs) {
    if (!dOcc) return fail(TBVH_E_INVALID, "tbvh_occluded_sharded_device: null output");
    return shardedDeviceQuery(scenes, nDev, (void* const*)dRays, nRays, dOcc, 0, 1e30f, kernelMs, dispatchMs, "tbvh_occluded_sharded_device");
}

int tbvh_bin_rays_device(tbvh_context* c, const void* dIn, void* dOut, uint64_t n, const float bounds6[6], uint32_t cellBits, uint32_t flags, uint32_t* dPerm) {
    if (!c || !bounds6 || ((!dIn || !dOut) && n)) return fail(TBVH_E_INVALID, "tbvh_bin_rays_device: null argument");
    if (dIn == dOut) return fail(TBVH_E_INVALID, "tbvh_bin_rays_device: the batch cannot be binned in place");
    if (cellBits > 6 || (flags & ~3u) || (flags & 3u) == 3u) return fail(TBVH_E_INVALID, "tbvh_bin_rays_device: cell_bits 0..6, flags 0, 1 or 2");
    if (n > 0xffffffffull) return fail(TBVH_E_INVALID, "tbvh_bin_rays_device: at most 2^32 - 1 rays per call");
    TBVH_ENTER(c);
    if (!n) return 0;
    size_t scanTemp = 0;
    const size_t need = ray_bin_scratch_bytes(n, cellBits, flags, &scanTemp);
    if (need > c->binScratch.count()) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->binScratch.alloc(need));
    }
    RayBinArgs a;
    for (int k = 0; k < 3; k++) {
        a.lo[k] = bounds6[k];
        const float ext = bounds6[3 + k] - bounds6[k];
        a.scale[k] = ext > 0 ? (float)(1u << cellBits) / ext : 0.f;
    }
    a.cellBits = cellBits; a.flags = flags;
    HIP_TRY(timedBegin(c));
    HIP_TRY(launch_ray_bin((const RayRec*)dIn, (RayRec*)dOut, dPerm, n, nullptr, a, c->binScratch, scanTemp, (uint32_t)c->numCUs * 16u, c->stream));
    HIP_TRY(timedEnd(c));
    return 0;
}

// ---- ray generators ----------------------------------------------------------------------

int tbvh_generate_primary_device(tbvh_context* c, const tbvh_camera* cam, void* dRays, uint64_t first, uint64_t n) {
    if (!c || !cam || (!dRays && n)) return fail(TBVH_E_INVALID, "tbvh_generate_primary_device: null argument");
    if (!cam->width || !cam->height || cam->width % 4 || cam->height % 4 || !cam->spp_x || !cam->spp_y)   // (width 0: k_gen_primary divides by width / 4)
        return fail(TBVH_E_INVALID, "camera: width/height must be positive multiples of 4, spp > 0");
    TBVH_ENTER(c);
    if (!n) return 0;
    CameraArgs a;
    memcpy(a.eye, cam->eye, 12); memcpy(a.p1, cam->p1, 12); memcpy(a.p2, cam->p2, 12); memcpy(a.p3, cam->p3, 12);
    a.width = cam->width; a.height = cam->height; a.sppX = cam->spp_x; a.sppY = cam->spp_y;
    launch_gen_primary(a, (RayRec*)dRays, first, n, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int tbvh_generate_bounce_device(tbvh_context* c, const void* dVerts, const void* dIn, void* dOut, uint64_t n, uint32_t seed) {
    if (!c || ((!dVerts || !dIn || !dOut) && n)) return fail(TBVH_E_INVALID, "tbvh_generate_bounce_device: null argument");
    TBVH_ENTER(c);
    if (!n) return 0;
    TriSource src; src.mode = 0; src.verts = (const float4*)dVerts;
    launch_gen_bounce(src, (const RayRec*)dIn, (RayRec*)dOut, n, seed, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int tbvh_generate_shadow_device(tbvh_context* c, const void* dIn, void* dOut, uint64_t n, const float light[3], float eps) {
    if (!c || !light || ((!dIn || !dOut) && n)) return fail(TBVH_E_INVALID, "tbvh_generate_shadow_device: null argument");
    TBVH_ENTER(c);
    if (!n) return 0;
    launch_gen_shadow((const RayRec*)dIn, (RayRec*)dOut, n, light[0], light[1], light[2], eps, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int tbvh_reset_hits_device(tbvh_context* c, void* dRays, uint64_t n, float tmax) {
    if (!c || (!dRays && n)) return fail(TBVH_E_INVALID, "tbvh_reset_hits_device: null argument");
    TBVH_ENTER(c);
    if (!n) return 0;
    launch_reset_hits((RayRec*)dRays, n, tmax, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
