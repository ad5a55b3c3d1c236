// capi_internal.h — what the translation units behind include/tinybvh_amd.h share: the context and scene objects, the error
// helper, and the few internal entry points that cross files (capi_context / capi_scene / capi_copies / capi_query / capi_wavefront / capi_host).
// Not installed; nothing outside tinybvh_amd/csrc includes it.
#pragma once
#include "../../include/tinybvh_amd.h"
#include "../../include/tinybvh_amd_debug.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "copy_policy.h"
#include "dev_buf.h"
#include "host_builder.h"
#include "kernels.h"
#include "launch_plan.h"
#include "overlap_lanes.h"
#include "probe_memory.h"
#include "ray_pool.h"
#include "tlas_plan.h"

using namespace tbvh;
using tbvh_capi::DevBuf;
using tbvh_capi::CopyKind;
using tbvh_capi::CopyPolicy;
using tbvh_capi::kCopyWide4;
using tbvh_capi::kCopyWide8;

static_assert(kLayoutBvhGpu == TBVH_LAYOUT_BVH_GPU && kLayoutBvh4Gpu == TBVH_LAYOUT_BVH4_GPU && kLayoutCwbvh == TBVH_LAYOUT_CWBVH,
              "kernels.h and the public header agree on the layout codes");
static_assert(tbvh_capi::kPlanLayoutCwbvh == TBVH_LAYOUT_CWBVH, "launch_plan.h and the public header agree on BVH8_CWBVH's code");
static_assert(tbvh_capi::kTlasLayoutSphere == TBVH_LAYOUT_BVH2_WALD && tbvh_capi::kTlasLayoutBvhGpu == TBVH_LAYOUT_BVH_GPU && tbvh_capi::kTlasLayoutBvh4Gpu == TBVH_LAYOUT_BVH4_GPU &&
              tbvh_capi::kTlasLayoutCwbvh == TBVH_LAYOUT_CWBVH && tbvh_capi::kTlasLayoutVoxel == TBVH_LAYOUT_VOXELSET, "tlas_plan.h and the public header agree on the layout codes");

namespace tbvh_capi {
int fail(int code, const char* fmt, ...);   // sets tbvh_last_error() of the calling thread, returns code
}  // namespace tbvh_capi

// A BVH_DOUBLE scene (capi_double.hip) answers tbvh_intersect_ex / tbvh_occluded_ex (and free / layout / bytes) only: every other entry point
// that takes a scene refuses it with this, before it touches the scene's memory or launches anything.
#define TBVH_REFUSE_DOUBLE(scene, who)                                                                                              \
    do {                                                                                                                            \
        if ((scene) && (scene)->layout == TBVH_LAYOUT_BVH_DOUBLE)                                                                   \
            return tbvh_capi::fail(TBVH_E_INVALID, "%s: a BVH_DOUBLE scene takes tbvh_intersect_ex / tbvh_occluded_ex only", who);   \
    } while (0)

// A VOXELSET scene (capi_voxel.hip) answers the ordinary queries (launchQuery) and can be a TLAS's BLAS; the entry points that have no
// voxel form refuse it with this, before they touch the scene's memory or launch anything.
#define TBVH_REFUSE_VOXEL(scene, who)                                                                                                   \
    do {                                                                                                                                \
        if ((scene) && (scene)->layout == TBVH_LAYOUT_VOXELSET)                                                                         \
            return tbvh_capi::fail(TBVH_E_INVALID, "%s: a VOXELSET scene takes the queries and can be a TLAS's BLAS; nothing else", who); \
    } while (0)

// A custom-geometry sphere BLAS (TBVH_LAYOUT_BVH2_WALD, capi_custom.hip) answers the ordinary queries (launchQuery) and can be a TLAS's BLAS; the
// entry points that have no sphere form refuse it with this, before they touch the scene's memory or launch anything.
#define TBVH_REFUSE_CUSTOM(scene, who)                                                                                                    \
    do {                                                                                                                                  \
        if ((scene) && (scene)->layout == TBVH_LAYOUT_BVH2_WALD)                                                                          \
            return tbvh_capi::fail(TBVH_E_INVALID, "%s: a sphere BLAS (custom geometry) takes the queries and can be a TLAS's BLAS; nothing else", who); \
    } while (0)

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail(TBVH_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct tbvh_context {
    // One lock per context: every entry point that touches the context (its stream position, staging buffers, ray-pool counter areas, event
    // ring, scenes) holds it, so host threads may share a context and a scene the way the reference's callers share a BVH
    // (tiny_bvh_speedtest.cpp:1077-1083 runs the const Intersect from 8 threads): calls on ONE context serialise — correct, not concurrent;
    // threads that want their queries to overlap use one context each (include/tiny_hip.h: tinyhip::Scene::ForThread).  Recursive: entry
    // points call each other (tbvh_upload_host -> tbvh_upload_cwbvh, the sharded calls -> the per-device ones).
    std::recursive_mutex mu;
    int device = 0;
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    // HIP-event timing: every timed operation (query, refit, build, ...) takes the next of kTimeRing event pairs, so a caller can enqueue many
    // operations back to back and read all their durations afterwards (tbvh_time_history) instead of synchronizing after each one
    // (tbvh_time_last_ms); ev0 / ev1 = the pair of the most recent operation.
    static constexpr uint32_t kTimeRing = 256;
    hipEvent_t evRing[kTimeRing][2] = {};
    bool evDone[kTimeRing] = {};
    int cohTunerMode = 0;         // TBVH_COHERENT_TUNER: 0 = measure per scene (default), 1 = always the deferred + gated schedule, 2 = always the strict one, 3 = always one traversal per wave
    uint64_t evSeq = 0;           // timed operations begun on this context
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    int numCUs = 0;
    uint32_t blocks = 0;          // persistent grid size (64-thread workgroups)
    DevBuf<uint32_t> spill;       // stack spill area
    uint32_t spillEntries = 0;    // 32-bit entries per lane
    DevBuf<unsigned long long> counter;     // status word, instrumentation counters
    uint32_t poolParts = 5;   // log2: 32 partitions
    bool embedTris = true;          // TBVH_EMBED_TRIS=0: the hybrid node copy without a triangle in each node's line (A/B: tools/ab_configs.py)
    bool incoherentCopies = true;   // TBVH_INCOHERENT_COPIES=0: no hybrid node copy / 64-byte triangle records (prepareIncoherentCopies)
    uint32_t expFlags = 0;     // tbvh_debug_set_flags: QueryArgs::flags of the next launches (experiments)
    bool skipTiming = false;   // launches enqueued by a stage loop of the library itself (the wavefront frame): no event pair per query
    bool lastProbed = false;   // the most recent query launch ran the coherence probe (tbvh_debug_last_probe)
    bool gridOverride = false;     // TBVH_BLOCKS_PER_CU / TBVH_RAYS_PER_BLOCK given: no per-scene adjustment
    uint64_t splitBelow = 12ull << 20;   // batches of fewer rays split their last rays over idle lanes; TBVH_SPLIT_RAYS=0 turns that off (tie order then reproducible run to run)
    uint32_t raysPerBlock = 128;   // small batches: one workgroup per this many rays (with split rays, profiles/r02_grid_sweep.txt: 96-128 best on 1 M-ray batches, +5 % over 192; flat at 4 M)
    DevBuf<uint32_t> pool;                  // ray-fetch counters: kPoolParts of them, 256 bytes apart (ray_pool.h), + the coherence probe's line; TWO such areas
    int poolCur = 0;              // the area the next launch draws from; its kernels zero the other one for the launch after (no memset in the stream)
    bool poolClean = false;       // both areas are known to be as that scheme leaves them (false: the next launch clears them itself)
    uint32_t* status = nullptr;   // (inside `counter`)
    // ---- two launch lanes (overlap_lanes.h; capi_query.hip: launchQuery) ----------------------------------------------------------------------
    // Lane 0 is `stream`, lane 1 a second stream of the context's own, made by the first launch that takes it.  Only the device-resident queries
    // (tbvh_intersect_device, tbvh_intersect_device_fresh, tbvh_occluded_device) ever take lane 1, and only while the context runs on its own
    // stream; every other entry point joins the lanes first (setDevice).  What above is per launch in flight belongs to lane 0 — `pool`, `poolCur`,
    // `poolClean`, `spill` — and lane 1 has its own here: the counter areas' zero-the-other-one scheme and the stack spill area assume that the
    // launches using them are serial, which holds within a lane only.
    struct Lane1 {
        hipStream_t stream = nullptr;
        DevBuf<uint32_t> pool, spill;
        int poolCur = 0;
        bool poolClean = false;
        bool unusable = false;      // the stream or an allocation failed: launches do not overlap on this context
    } lane1;
    bool overlap = true;            // TBVH_OVERLAP=0 / tbvh_context_set_overlap(ctx, 0): every launch on lane 0, as before the lanes
    tbvh_capi::LaneBook book;       // launches in flight on each lane (a record's slot = its event pair in evRing)
    hipEvent_t evBase = nullptr;    // lane 0's position ahead of its in-flight query launches: what a launch on lane 1 waits for (generators, uploads, refits enqueued earlier)
    hipEvent_t lane1Last = nullptr; // end event of lane 1's most recent launch (one of evRing)
    // The other lane's next launch starts after the start of one of a lane's last launches (LaneBook::gate names it by its evSeq number; its start event
    // is evRing[number % kTimeRing][0] for as long as fewer than kTimeRing timed operations have begun since: ringHolds).
    int overlapDepth = 1;           // TBVH_OVERLAP_DEPTH / tbvh_debug_set_overlap_depth: how many launches one lane may start ahead of the other (1 or 2).  2 measured
                                    // +1.3 % on the bench alone and nothing on top of the probe memory (profiles/r09_runahead.txt): it stays a setting, off
    bool ringHolds(uint64_t seq) const { return seq < evSeq && evSeq - seq <= kTimeRing; }
    // ---- what the coherence probe said about a buffer's last launches (probe_memory.h; capi_query.hip: launchQuery) -----------------------------
    bool probeMemoryOn = true;      // TBVH_PROBE_MEMORY=0 / tbvh_debug_set_probe_memory(ctx, 0): every probed launch is two flavors
    tbvh_capi::ProbeMemory probeMemory;
    uint32_t* probeSlots = nullptr; // host-coherent pinned memory, two words per entry of evRing: the probe counts of the launch with that event pair, stored by its block 0
    bool probeSlotsFailed = false;
    uint64_t soloLaunches = 0, probeVerdicts = 0;   // tbvh_debug_probe_memory_stats
    bool lane1Dirty = false;        // lane 1 holds launches lane 0 has not waited for
    bool lane0Touched = true;       // something other than an overlappable launch went onto lane 0 since evBase was recorded
    bool lane1SawBase = false;      // lane 1 waits for evBase as recorded now
    bool serialiseNext = false;     // the previous launch was one a CohTuner measured: this one does not overlap with it either
    int lastProbedLane = 0;
    uint32_t chain = 1;             // counts the joins: launches of one chain may have overlapped each other
    uint32_t evChain[kTimeRing] = {};   // per timed operation: the chain of an overlappable launch, 0 for everything else (tbvh_time_history)
    uint64_t lane1Launches = 0, laneJoins = 0;   // tbvh_debug_overlap_stats
    DevBuf<RayRec> stageRays;     // staging for host-array queries
    DevBuf<uint8_t> stageOcc;
    // host-array queries of more than a few 10 k rays go through pinned staging in chunks: worker threads gather the
    // 64-byte prefixes of the caller's records into a pinned buffer while the previous chunk is in flight (a pageable
    // hipMemcpy2D moves ~9 GB/s because one CPU thread does the staging copy), and the 20 result bytes per ray come back
    // packed (k_pack_hits) and are scattered by the same workers
    struct HostPipe* pipe = nullptr;
    // page-locked host memory handed out by tbvh_pinned_malloc: a packed (64-byte) ray array inside such a range goes up by DMA straight from there,
    // without the packing pass through the library's pinned ring (capi_query.hip: hostQuery)
    struct PinnedRange { char* host; uint64_t bytes; };
    float hostQueryMs = -1.f;     // device time of the most recent host-array query (the sum over its groups' launches) ...
    uint64_t hostQuerySeq = ~0ull; // ... valid while no later operation was timed (evSeq still equals this)
    std::vector<PinnedRange> pinned;
    DevBuf<void> binScratch;      // tbvh_bin_rays_device
    uint32_t sahSmallSubtree = 64;   // (sahbuild.h: kSahSmallSubtreeDefault) tbvh_debug_set_sah_small_subtree
    uint32_t sahOneGroup = 3000;     // (sahbuild.h: kSahOneGroupDefault) tbvh_debug_set_sah_one_group
    std::vector<tbvh_scene*> scenes;
    std::vector<struct tbvh_pose*> poses;   // (capi_pose.hip) the poses made on this context: tbvh_shutdown frees those the caller has not
    std::vector<struct tbvh_scenegraph*> graphs;   // (capi_scenegraph.hip) likewise the scene graphs
    std::vector<struct tbvh_shading*> shadings;   // (capi_shade.hip) likewise the shading tables
    std::vector<struct tbvh_sky*> skies;          // (capi_viewer.hip) likewise the sky domes ...
    std::vector<struct tbvh_viewer*> viewers;     // ... and the viewer frames
    // (capi_omm.hip) the texture descriptors of a bake go up through a pinned area, in stream order, into ommDesc: a device-resident bake stays asynchronous;
    // the area is reused once the previous bake's copy has left it (ommEv)
    DevBuf<void> ommDesc;
    void* ommPin = nullptr;
    size_t ommPinBytes = 0;
    hipEvent_t ommEv = nullptr;
    bool ommPinUsed = false;
};

// Which schedule runs COHERENT batches of a two-flavor launch on this scene: the deferred-triangles + gated schedule on a third more waves
// (kernels_cwbvh.hip: PROBED == 3; +1 ... +8 % on camera and shadow rays of the street, foliage, soup stand-ins) or the strict one (PROBED == 4; +10 %
// on camera rays of the atrium generator at 1 M triangles, whose big occluders make every node visited ahead of a pending triangle test wasted work:
// profiles/r04_sensitivity.txt).  No static property of a blob told the two apart, so the library measures: while undecided the launches alternate
// between the two, an event between the two kernels times the first one, and after two coherent samples of each the faster (by 3 %) stays.
struct CohTuner {
    int decided = 0;                    // 0 measuring, 1 deferred + gated, 2 strict, 3 one traversal per wave (kernels_cwbvh_packet.hip)
    bool pinned = false;                // `decided` came from the caller (tbvh_scene_set_schedule_hint): not measured, not reset by a topology change
    uint32_t launches = 0;
    uint64_t refRays = 0;               // size of the first coherent batch sampled: only batches within 3/4 ... 4/3 of it are compared
    static constexpr int kModes = 3;
    uint32_t n[kModes] = {0, 0, 0};             // coherent-verdict samples per schedule
    float best[kModes] = {1e30f, 1e30f, 1e30f};     // ns per ray of the first kernel: best sample per schedule (other work on the GPU only ever ADDS time: the minimum is the robust statistic)
    // a launch being measured: the tuner's OWN event pair around the first kernel (so it measures with tbvh_set_timing(0) as well)
    struct Pending { hipEvent_t e0, e1; int mode; uint64_t rays; };
    std::vector<Pending> pending;
    static constexpr uint32_t kSamples = 3;   // per schedule, before the faster (by 3 %) stays
    void drop_pending() { for (Pending& p : pending) { hipEventDestroy(p.e0); hipEventDestroy(p.e1); } pending.clear(); }
    // (capi_query.hip) the measured launches that have finished since: their times go into n / best; first kernels that left within `minMs` (the probe found
    // the batch incoherent) and batches of another size than the first one sampled are not samples
    void harvest(float minMs);
    // once every schedule has its samples: `decided` is set.  packetOrStrict: the scene's per-lane kernel runs strict whatever (scenes under 48 MB and beyond
    // 384 MB) — the packet kernel must win by `margin` AND by 15 us per launch, which is what the second kernel of a probed launch costs
    void settle(bool packetOrStrict, float margin);
    int least_sampled() const;   // the schedule with the fewest samples taken or in flight
};

// The derived copies of a BLAS in ANOTHER layout, each a scene of its own that this one owns (capi_copies.hip makes, drops, refits and selects them; not
// listed in the context's scene table).  copy8: a BVH_GPU / BVH4_GPU tree collapsed 8-wide into the BVH8_CWBVH format, made by the first query, kept current
// by update / refit / micromap calls and traced INSTEAD of `nodes` by the queries on the scene: hit records do not depend on the layout (device_common.h:
// hit_wins), and the compressed wide kernels trace the same rays 1.6-2.9 x faster than the 2-wide one (profiles/r06_bvh2.txt).  copy4: a BVH_GPU /
// BVH8_CWBVH BLAS in the BVH4_GPU format, made when a TLAS is uploaded over it: under a TLAS k_tlas4 is the fastest kernel for closest hits (1000 instances,
// camera rays: 4650 MRays/s against 4190 through BVH8_CWBVH BLASes and 3840 through BVH_GPU ones), k_tlas8 for any-hit queries (blasView).
struct WideCopies {
    tbvh_scene* copy8 = nullptr;
    tbvh_scene* copy4 = nullptr;
    bool tried8 = false, tried4 = false;   // the copy was made, or found unwanted / impossible: not tried again
    bool tlasOnly = false;                 // copy8 is a small one made for the TLASes over this scene: the scene's own queries keep the uploaded nodes
    CopyPolicy policy;                     // when they are dropped and come back (copy_policy.h)
    uint8_t live() const { return (uint8_t)((copy8 ? kCopyWide8 : 0) | (copy4 ? kCopyWide4 : 0)); }
    uint8_t pending() const { return policy.pendingCopies; }
};

// The re-layouts of a BVH8_CWBVH scene's own arrays (capi_copies.hip; launchCwbvhKernels picks among them)
struct CwbvhLayouts {
    DevBuf<float4> padded;       // the same nodes padded to one 128-byte line each (padCwbvhIfLarge: node arrays beyond the Infinity Cache)
    DevBuf<float4> hybrid;       // the same nodes in surface-area priority order, the first `packed` packed, the others one per line (cwbvh_node.h: kNodeHybrid)
    DevBuf<uint32_t> perm;       // device: position of node i in `hybrid`
    DevBuf<float4> trisPadded;   // triangle records padded to 64 bytes
    uint32_t packed = 0;         // (QueryArgs::hybridK)
    bool tried = false;          // the incoherent-batch copies were built, or found impossible / unwanted: launchQuery does not try again
    bool levelOrder = false;     // the node array is in level order (made on the device): the hybrid copy needs no renumbering
};

// What only a TLAS holds (capi_scene.hip makes, classifies, updates and rebuilds it; a BVH_DOUBLE TLAS — capi_double.hip — uses the counts and the BLAS
// list).  WHICH arrays each BLAS is entered through, which wide trees are kept and which kernel serves a query is `plan` (tlas_plan.h), stated again by
// reclassifyTlas whenever a fact it reads changes; what the scene reports as its bytes is derived from what is held here (sceneBytes).
struct TlasState {
    DevBuf<uint32_t> tlasIdx;
    DevBuf<float4> instances;   // 12 per instance
    uint64_t nInst = 0, nBlas = 0, nTlasNodes = 0, nTlasIdx = 0;
    std::vector<tbvh_scene*> blasList;   // its BLASes, in blasIdx order
    bool blasSpheres = false;         // some BLAS is a sphere BLAS (capi_custom.hip): every query takes the flat loop with the sphere step, BLASes in their own layouts
    bool anyHitSeen = false;          // the TLAS has had an any-hit query: only then do its BVH4_GPU BLASes get their 8-wide copies and the second wide tree is kept (a frame loop that only
                                      // ever calls Intersect pays for neither: per frame the second tree's rebuild and the copies' refit cost 0.27 ms at 1000 instances)
    bool blasRecopyPending = false;   // the copies of some BLAS are waiting to be made again (copy_policy.h)
    // the plan in force, the views it chose per BLAS ([0] closest-hit, [1] any-hit) and the descriptor tables uploaded for them; blasDescAny only while any-hit
    // queries have a class of their own (BVH4_GPU BLASes: their own stream for closest hits — k_tlas4 —, their 8-wide copies for IsOccluded — k_tlas8, + 28 % on 1000 instances)
    tbvh_capi::TlasPlan plan;
    std::vector<tbvh_capi::TlasView> view[2];
    DevBuf<BlasDesc> blasDesc, blasDescAny;
    // the same TLAS collapsed 4-wide in the BVH4_GPU node format (kernels_tlas4.hip) and 8-wide in the BVH8_CWBVH one (kernels_tlas8.hip), whichever the plan
    // wants, kept current by every upload / update / device rebuild; one scratch area for both builds
    DevBuf<float4> tlas4;             // count(): blocks
    DevBuf<float4> tlas8;             // 5 per node: count() / 5 = nodes the wide tree may have (allocated after tlas8Refs: never there without them)
    DevBuf<uint32_t> tlas8Refs;       // instance references: the same number
    DevBuf<void> tlas4Scratch;
    // device-side TLAS rebuild (kernels_tlasbuild.hip)
    DevBuf<float> blasBounds;         // 6 floats per BLAS
    // tbvh_tlas_set_builder: 0 = LBVH, 2 = the reference's SAH tree (kernels_sahbuild.hip over the instance records, then the device Aila-Laine encode).
    // The SAH build keeps its Wald nodes (2 n) and its scratch here, sized for tlasSahFor instances: no allocation per frame; sceneBytes counts them.
    int tlasBuilder = 0;
    DevBuf<float4> tlasWald;
    DevBuf<void> tlasSah;
    uint64_t tlasSahFor = 0;
    size_t tlasSahSort = 0, tlasSahScan = 0;
    DevBuf<float> xformStage;         // staged transforms (16 floats per instance) when the caller passes host memory
};

struct tbvh_scene {
    tbvh_context* ctx = nullptr;
    int layout = 0;
    int variant = 0;
    DevBuf<float4> nodes;      // BVH_GPU nodes / BVH4 stream / CWBVH nodes
    DevBuf<float4> tris;       // BVH_GPU gathered tris / CWBVH tris
    CwbvhLayouts cw;
    CohTuner cohTuner[2][4];    // [any-hit][batch-size class: < 6 M, < 12 M, more rays; 3 = 768 k .. 1.5 M rays on a scene under 48 MB]: which schedule wins can depend on the batch size (the tail of a launch weighs differently)
    uint8_t cohLastClass[2] = {2, 2};   // the class of the most recent two-flavor launch (tbvh_debug_coherent_schedule reports that one)
    uint32_t nNodes = 0;
    uint64_t nNodeBlocks = 0, nTriBlocks = 0;
    uint64_t capNodeBlocks = 0, capTriBlocks = 0;   // what the allocations hold (tbvh_update_*: a re-converted blob of at most this size goes in place)
    uint64_t topoHash = 0;       // CWBVH: hash of every node's (imask, child base): an update with the same topology keeps the hybrid copy's numbering
    // TLAS (layout = BVH_GPU nodes in `nodes`; a BVH_DOUBLE TLAS keeps its counts and BLAS list in `tlas` too)
    bool isTlas = false;
    TlasState tlas;
    // BLAS <-> TLAS references: a TLAS snapshots its BLASes' device pointers (BlasDesc), so a BLAS knows the TLASes that
    // use it (their descriptors are refreshed when its opacity maps change) and outlives them (tbvh_free_scene on a BLAS
    // that is still referenced only marks it; the memory goes when the last TLAS over it is freed)
    std::vector<tbvh_scene*> usedBy;     // BLAS: the TLASes built over it (one entry per reference)
    bool zombie = false;                 // BLAS: freed by the caller while still referenced
    // scratch of the device builds that sort: a TLAS's rebuild (fp32 and fp64) and a sphere BLAS's build share it, so it is the scene's, not the TLAS's
    DevBuf<void> buildScratch;
    size_t sortTempBytes = 0;
    uint64_t buildScratchFor = 0;     // instance / sphere count the scratch was sized for
    // device-side BLAS refit (kernels_refit.hip)
    DevBuf<void> refitScratch;
    std::vector<uint32_t> b4Levels;   // BVH4_GPU: first node of every tree level in the item list (filled by the first refit)
    DevBuf<void> vertStage;           // staged vertices when the caller passes host memory (strided meshes: sized in bytes)
    // opacity micromaps (BVHBase::SetOpacityMicroMaps): what the kernels read is a plain pointer on every scene — a derived copy (WideCopies)
    // shares its owner's maps —, the allocation belongs to the scene they were set on
    uint32_t* opmap = nullptr;
    DevBuf<uint32_t> opmapOwn;
    uint32_t opmapN = 0;
    // a scene made from an INDEXED mesh (tbvh_*_mesh with indices) keeps its own device copy of the index buffer, 12 bytes per triangle, counted by
    // sceneBytes: tbvh_refit_mesh with indices == NULL then means "the indices the scene holds" — the per-frame call of an animated mesh passes the
    // shared vertices only.  The derived copies (WideCopies) hold none: their refit is handed the owner's source.
    DevBuf<uint32_t> meshIdx;
    uint64_t meshIdxTris = 0;
    DevBuf<uint32_t> idxStage;           // staged host indices of tbvh_intersect_spheres_mesh (a per-frame query: no allocation per call)
    // the scene's triangle test (tbvh_set_triangle_test, capi_watertight.hip).  A watertight scene holds its own copy of the caller's vertices, 3 float4 per
    // triangle in primitive order (sceneBytes counts it; refits write it again): the watertight kernels fetch a triangle through its record's primitive
    // index.  Like the opacity maps, what the kernels read is a plain pointer on every scene: an 8-wide copy shares its owner's.
    int triTest = 0;
    const float4* wtVerts = nullptr;
    uint64_t wtTris = 0;
    DevBuf<float4> wtVertsOwn;
    WideCopies copies;
    uint64_t raysTraced = 0;            // rays of every query launched on this scene (a TLAS counts its own): what a refit weighs the copies' refit against
    // a sphere BLAS that moves (capi_custom.hip: tbvh_build_device_custom_spheres / tbvh_rebuild_custom_spheres_device / tbvh_refit_custom_spheres): the
    // sphere count and the builder a rebuild repeats (an uploaded scene: LBVH, one sphere per leaf).  The build keeps its scratch in buildScratch
    // (sized for buildScratchFor spheres) and its primIdx here, the refit its pass words in refitScratch, host spheres are staged in vertStage: no
    // allocation per frame; sceneBytes counts them all.
    uint64_t sphN = 0;
    int sphBuilder = 0;                  // 0 LBVH, 1 PLOC, 2 SAH (tbvh_build_device_custom_spheres_sah; sphMaxLeaf 0 = the leaves BVH::Build makes)
    uint32_t sphMaxLeaf = 1, sphRadius = 16;
    size_t scanTempBytes = 0;
    DevBuf<uint32_t> sphIdx;
    // BVH_DOUBLE scenes that move (capi_double.hip).  A TLAS: what the parts of its one allocation hold (tlasParts lays them out by these, so a smaller
    // tree goes in place); the rebuild keeps its scratch in buildScratch (sized for buildScratchFor instances).  A BLAS: its triangle count, and from the
    // first refit on parent[] | leaf list | flags in refitScratch (dblLeaves leaves); host vertices are staged in vertStage.  sceneBytes counts them all.
    // a voxel set that is edited (capi_voxel_edit.hip): `nodes` holds [top 16 | grid 32768 | bricks capacity x 512] and nNodes the USED bricks; the batched
    // Set keeps its fixed-size work area (first record per grid cell, the sort's arrays, counters) in voxWork, one winner word per voxel of the pool in
    // voxWinner (all zero between calls) and staged host records in voxStage.  sceneBytes counts all three.
    DevBuf<uint32_t> voxWork, voxWinner, voxStage;
    size_t voxSortTemp = 0;
    uint64_t dblCapNodes = 0, dblCapIdx = 0, dblCapInst = 0;
    uint64_t dblTris = 0, dblRecs = 0;
    uint32_t dblLeaves = 0;
    // a BVH_DOUBLE BLAS over custom geometry (capi_double.hip, custom_sphere_dbl.h): `tris` holds 48-byte sphere records, dblRecs of them over dblTris
    // spheres; a device build sizes `nodes` / `tris` for the 2 n - 1 nodes / n records of its tree and keeps its scratch in buildScratch, host spheres
    // are staged in vertStage.  sceneBytes counts the allocations, so a rebuild in place leaves the scene's bytes as they were.
    bool dblSpheres = false;
};

struct BLASInstanceCheck { float m[32]; float mn[3]; uint32_t blasIdx; float mx[3]; uint32_t mask; uint32_t pad[8]; };
static_assert(sizeof(BLASInstanceCheck) == 192, "BLASInstance is 192 bytes");

struct tbvh_hostbvh {
    int layout = 0;
    BVH2 bvh2;
    std::vector<NodeAL> al;
    std::vector<Vec4> blocksA, blocksB;
    std::vector<NodeDbl> dnodes;     // TBVH_LAYOUT_BVH_DOUBLE (capi_double.hip): BVH_Double::bvhNode ...
    std::vector<uint64_t> didx;      // ... and primIdx (TLAS: instance indices)
    std::vector<uint32_t> vgrid, vbricks, vtop;   // TBVH_LAYOUT_VOXELSET (capi_voxel.hip): VoxelSet's grid, brick pool (used bricks) and top grid
};

struct HostPipe {
    static constexpr uint64_t kChunk = 1ull << 18;   // rays per chunk: 16 MB up, 5 MB down
    void* pinUp[2] = {nullptr, nullptr};
    hipEvent_t evUp[2] = {nullptr, nullptr};
    hipStream_t down = nullptr;   // the results' way back: pack kernel + device-to-host copies, beside the uploads and kernels on the context's stream
    hipEvent_t evKernel = nullptr;
    std::vector<hipEvent_t> evGroup;   // group g's results have landed in pinDown
    DevBuf<uint32_t> packed;      // device: 5 dwords per ray (bytes 44..63 of the record)
    void* pinDown = nullptr;      // pinned host: the same, for the whole batch
    // a small persistent worker pool: parallel_for(n, fn) runs fn(part, parts) on every worker and the caller
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable cvWork, cvDone;
    std::function<void(uint32_t, uint32_t)> job;
    uint64_t generation = 0;
    uint32_t pending = 0;
    bool quit = false;
    void start(uint32_t nThreads) {
        for (uint32_t t = 0; t < nThreads; t++)
            workers.emplace_back([this, t, nThreads] {
                uint64_t seen = 0;
                for (;;) {
                    std::function<void(uint32_t, uint32_t)> f;
                    {
                        std::unique_lock<std::mutex> lk(m);
                        cvWork.wait(lk, [&] { return quit || generation != seen; });
                        if (quit) return;
                        seen = generation; f = job;
                    }
                    f(t + 1, nThreads + 1);
                    {
                        std::lock_guard<std::mutex> lk(m);
                        if (--pending == 0) cvDone.notify_all();
                    }
                }
            });
    }
    void parallel_for(uint64_t items, const std::function<void(uint32_t, uint32_t)>& f) {
        if (items < 16384 || workers.empty()) { f(0, 1); return; }   // (a few thousand records: waking the workers costs more than the copy)
        {
            std::lock_guard<std::mutex> lk(m);
            job = f; pending = (uint32_t)workers.size(); generation++;
        }
        cvWork.notify_all();
        f(0, (uint32_t)workers.size() + 1);
        std::unique_lock<std::mutex> lk(m);
        cvDone.wait(lk, [&] { return pending == 0; });
    }
    ~HostPipe() {
        { std::lock_guard<std::mutex> lk(m); quit = true; }
        cvWork.notify_all();
        for (auto& w : workers) w.join();
        for (int i = 0; i < 2; i++) {
            if (pinUp[i]) hipHostFree(pinUp[i]);
            if (evUp[i]) hipEventDestroy(evUp[i]);
        }
        for (hipEvent_t e : evGroup) hipEventDestroy(e);
        if (evKernel) hipEventDestroy(evKernel);
        if (down) hipStreamDestroy(down);
        if (pinDown) hipHostFree(pinDown);
    }
};

namespace tbvh_capi {
int setDevice(tbvh_context* c);
// first statement of an entry point once its arguments are known to be non-null: take the context's lock for the rest of the call, make its device current
#define TBVH_LOCK(ctxptr) std::lock_guard<std::recursive_mutex> ctx_lock_((ctxptr)->mu)
#define TBVH_ENTER(ctxptr) std::lock_guard<std::recursive_mutex> ctx_lock_((ctxptr)->mu); if (int r_ = tbvh_capi::setDevice(ctxptr)) return r_
// the common entry path: the device is current and lane 0 comes after everything enqueued on lane 1 (joinLanes)
int joinLanes(tbvh_context* c);
hipError_t timedBegin(tbvh_context* c, hipStream_t lane = nullptr);   // next event pair of the ring, start event recorded on the context's stream (or on `lane`)
hipError_t timedEnd(tbvh_context* c, hipStream_t lane = nullptr);     // end event recorded; the operation counts as timed
float timedMs(tbvh_context* c, uint64_t seq);   // what timed operation `seq` (counted from 0; still in the ring, its events reached) reports: see tbvh_time_history
// one query launch (probe-in-kernel + traversal kernel(s)) on the context's stream; asynchronous.  nDev: batch size in device memory (wavefront queues).
// mayOverlap: the launch may take lane 1 (the three device-resident query entry points pass it; everything else stays on lane 0 behind a join)
int launchQuery(tbvh_scene* s, tbvh::RayRec* d_rays, uint64_t n, uint8_t* d_occ, bool fresh = false, float freshTmax = 1e30f,
                const unsigned long long* nDev = nullptr, bool mayOverlap = false);
int checkStatus(tbvh_context* c);   // synchronizes the stream, turns the device status word into an error code
int ensureStage(tbvh_context* c, uint64_t n);      // (capi_query.hip) the host-array staging buffers hold at least n ray records ...
int ensureStageOcc(tbvh_context* c, uint64_t n);   // ... and n any-hit result bytes
tbvh_scene* newScene(tbvh_context* c, int layout);
// (capi_scene.hip) what scene s costs on the device, as a function of what it holds NOW: the one list of terms behind tbvh_scene_device_bytes, planLaunch's
// blobBytes and tbvh_debug_scene_bytes.  word[0..6] are counted, word[7] is held but not counted (the words: include/tinybvh_amd_debug.h).  Follows the
// scene's wide copies: the caller holds the context's lock.
struct SceneBytes { uint64_t word[8]; };
SceneBytes sceneBytesByWord(const tbvh_scene* s);
uint64_t sceneBytes(const tbvh_scene* s);   // word[0] + ... + word[6]
TlasFacts tlasFactsNow(const tbvh_scene* s, std::vector<TlasBlasFacts>& blas);   // (capi_scene.hip) the facts of TLAS s as they are now; `blas` holds the per-BLAS part
int reclassifyTlas(tbvh_scene* t);   // (capi_scene.hip) the plan (tlas_plan.h), descriptors and wide trees of a TLAS from its BLASes as they are now
// ---- derived copies (capi_copies.hip): WideCopies and CwbvhLayouts are made, dropped, refitted and selected there and nowhere else -----------
uint64_t cwbvhTopologyHash(const tbvh::Vec4* nodes, uint32_t nNodes);
int prepareIncoherentCopies(tbvh_scene* s);   // launchQuery: a probed launch on the scene (the first one builds, or finds them unwanted)
int rederiveCwbvhLayouts(tbvh_scene* s);      // the node boxes or triangle records changed in place, the tree (s->nNodes, s->nTriBlocks) did not; asynchronous
int resetCwbvhLayouts(tbvh_scene* s, bool levelOrder = false);   // a new tree in the scene's arrays (upload, device conversion, update): none but the padded nodes of a large one
void freeCopy(tbvh_scene* s, CopyKind kind);
void makeCopyOnce(tbvh_scene* b, CopyKind kind);   // the copy of this kind, unless it was tried before, b's layout has none or b pins its uploaded nodes (tbvh_set_variant)
void dropCopiesAfterUpdate(tbvh_scene* s);   // tbvh_update_*: see copy_policy.h
void countQueryForRecopy(tbvh_scene* s);     // ... and the query side of it (launchQuery)
tbvh_scene* wideCopyForQuery(tbvh_scene* s);   // the 8-wide copy the scene's own queries run on, or nullptr: they run on s
tbvh_scene* tunedScene(tbvh_scene* s);         // the scene whose CohTuner decides for queries on s: its 8-wide copy if it has one
void shareOpacityMaps(tbvh_scene* s);          // the copies read the owner's maps
void shareTriangleTest(tbvh_scene* s);         // ... and the owner's triangle test and vertices (capi_watertight.hip)
int ensureWatertightCopy(tbvh_scene* s);       // (capi_copies.hip) a watertight BVH_GPU / BVH4_GPU scene is traced through its 8-wide copy whatever its size: made now if it is not there
int refreshWatertightVerts(tbvh_scene* s, const tbvh::MeshSrc& src);   // (capi_watertight.hip) tail of a refit: a watertight scene's vertices are src's from here on
int refitCopies(tbvh_scene* s, const tbvh::MeshSrc& src);   // tail of a refit of s: its copies follow in place, or go (CopyPolicy::refit)
TlasBlasFacts tlasBlasFacts(const tbvh_scene* b);                         // what tlas_plan.h reads of BLAS b
const tbvh_scene* blasView(const tbvh_scene* b, TlasView v);              // the scene whose arrays a TLAS enters b through under view v
// f(t) for each distinct TLAS t over BLAS b (usedBy holds one entry per reference), until one returns non-zero: that value, or 0
template <class F>
int forEachTlasOver(tbvh_scene* b, F f) {
    for (size_t i = 0; i < b->usedBy.size(); i++) {
        bool seen = false;
        for (size_t k = 0; k < i; k++) seen |= b->usedBy[k] == b->usedBy[i];
        if (!seen) if (int r = f(b->usedBy[i])) return r;
    }
    return 0;
}
// ---- vertex sources (capi_mesh.hip): tbvh_mesh of the public header -> MeshSrc of the kernels (mesh_source.h) ------------------------------
int checkMesh(const tbvh_mesh* m, const char* who, bool indicesMayBeHeld = false);   // the header's validation rules; host indices are range-checked here, before anything is allocated
tbvh_mesh flatMesh(const void* verts16, uint64_t nTris, int onDevice);   // what (verts16, n_tris) of the flat entry points mean
uint64_t meshVertexBytes(const tbvh_mesh& m);                          // bytes of the vertex array that may be read (the last vertex: 12 unless the stride is 16)
// a mesh as the kernels see it: device-resident arrays are used in place, host arrays are copied into allocations this object owns (asynchronous on the
// context's stream: synchronise before the caller's arrays may change and before this object goes)
struct DeviceMesh {
    tbvh::MeshSrc src;
    DevBuf<void> ownVerts;
    DevBuf<uint32_t> ownIdx;
};
int stageMesh(tbvh_context* c, const tbvh_mesh& m, DeviceMesh& out);
int keepMeshIndices(tbvh_scene* s, const tbvh::MeshSrc& src);          // the scene's own copy of src.indices (no-op without indices); device to device, asynchronous
// (capi_scene.hip) BVH2 on the device -> a new BVH8_CWBVH / BVH4_GPU scene; the wide copies are made by it too
int convertDeviceImpl(tbvh_context* c, int layout, const float4* dN2, uint64_t nNodes2, const uint32_t* dIdx, uint64_t nIdx, const tbvh::MeshSrc& dV, tbvh_scene** out);
int refitDeviceSource(tbvh_scene* s, const tbvh::MeshSrc& src);        // (capi_scene.hip) tbvh_refit / tbvh_refit_mesh once the source is on the device
int hostBuildImpl(const tbvh::HostMesh& mesh, uint64_t nTris, int layout, const tbvh_build_params* p, tbvh_hostbvh** out);   // (capi_host.hip) tbvh_host_build / _mesh
int checkSphereScene(tbvh_scene* s, const char* who);   // (capi_sphere.hip) the refusals a sphere query makes before it looks at anything else
int launchSpheres(tbvh_scene* s, const float4* dSpheres, uint64_t n, const tbvh::MeshSrc& verts, uint8_t* dHit);   // (capi_sphere.hip)
// (capi_scene.hip) the two halves of tbvh_set_opacity_micromaps, for tbvh_bake_set_opacity_micromaps (capi_omm.hip), which fills the buffer in place:
// room for nTris maps of N x N bits plus the padding the traversal's index may read (cleared, on the context's stream), and the swap that makes a filled
// buffer the scene's maps (N == 0 with an empty buffer: none) — derived copies and the TLASes over the scene follow, the old maps go
int allocOpacityMaps(tbvh_context* c, uint32_t N, uint64_t nTris, const char* who, DevBuf<uint32_t>& fresh, uint64_t* wordsOut);
int installOpacityMaps(tbvh_scene* s, DevBuf<uint32_t>&& fresh, uint32_t N);
void freeOmmStagingOf(tbvh_context* c);   // (capi_omm.hip) tbvh_shutdown: the pinned area and the event of the texture-descriptor upload
void freeGraphsOf(tbvh_context* c);   // (capi_scenegraph.hip) likewise
void freePosesOf(tbvh_context* c);   // (capi_pose.hip) tbvh_shutdown: the context's stream is idle, its device current
void freeShadingsOf(tbvh_context* c);   // (capi_shade.hip) likewise
// (capi_shade.hip) what a pose with FatTri records attached needs of a shading table: its context, and a slot's records as they are now (nullptr / 0: none)
tbvh_context* shadingContext(const struct tbvh_shading* sh);
void shadingSlotRecords(const struct tbvh_shading* sh, uint32_t slot, float4** tris, uint64_t* nTris);
void detachPosesFrom(tbvh_context* c, const struct tbvh_shading* sh);   // (capi_pose.hip) the table goes: the poses attached to it pose vertices only from here on
// (capi_shade.hip) what a viewer frame needs of a shading table: the shading kernel over records on the device (nDev: their count in device memory, or null),
// not timed, and the material table for the gltf alpha rule
void shadingLaunch(const struct tbvh_shading* sh, tbvh_scene* s, const void* dRays, uint64_t n, uint32_t strideBytes, void* dOut48, const unsigned long long* nDev);
void shadingMaterials(const struct tbvh_shading* sh, const struct tbvh::ShadeMat** mats, uint32_t* nMats, uint32_t* nTex, bool* anyColorTexture);
void freeViewersOf(tbvh_context* c);   // (capi_viewer.hip) tbvh_shutdown: the sky domes and viewer frames still alive
}  // namespace tbvh_capi
