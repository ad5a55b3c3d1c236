// capi_context.hip — contexts, streams, timing, debug knobs, device buffers and the ceilings bench.py measures (include/tinybvh_amd.h).
#include "capi_internal.h"
#include "packet_cull.h"
#include "device_common.h"
#include "lbvh.h"
#include "sahbuild.h"
#include "sbvhbuild.h"

using namespace tbvh;
using namespace tbvh_capi;

namespace {
thread_local char g_err[512] = "";
}  // namespace

namespace tbvh_capi {
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

// Lane 0 waits for lane 1's last launch; from here on nothing that is enqueued on either lane can pass a launch enqueued before.  (Lane 1's next
// launch waits for lane 0's position in turn: lane0Touched.)  Called by every entry point through setDevice; a launch that may overlap skips it.
int joinLanes(tbvh_context* c) {
    if (c->lane1Dirty) {
        HIP_TRY(hipStreamWaitEvent(c->stream, c->lane1Last, 0));
        c->lane1Dirty = false;
        c->laneJoins++;
    }
    c->book.joined();
    c->lane0Touched = true;
    c->chain++;
    if (!c->chain) c->chain = 1;
    return 0;
}
int setDevice(tbvh_context* c) {
    HIP_TRY(hipSetDevice(c->device));
    return joinLanes(c);
}
hipError_t timedBegin(tbvh_context* c, hipStream_t lane) {
    if (c->skipTiming) return hipSuccess;
    const uint32_t slot = (uint32_t)(c->evSeq % tbvh_context::kTimeRing);
    for (int k = 0; k < 2; k++)
        if (!c->evRing[slot][k]) { const hipError_t e = hipEventCreate(&c->evRing[slot][k]); if (e != hipSuccess) return e; }
    c->evDone[slot] = false;
    c->evChain[slot] = 0;
    c->ev0 = c->evRing[slot][0]; c->ev1 = c->evRing[slot][1];
    c->evSeq++;
    return hipEventRecord(c->ev0, lane ? lane : c->stream);
}
hipError_t timedEnd(tbvh_context* c, hipStream_t lane) {
    if (c->skipTiming) return hipSuccess;
    const hipError_t e = hipEventRecord(c->ev1, lane ? lane : c->stream);
    if (e == hipSuccess && c->evSeq) { c->evDone[(c->evSeq - 1) % tbvh_context::kTimeRing] = true; c->timed = true; }
    return e;
}
// A serial operation reports its own interval, start event to end event.  A launch that may have overlapped its neighbours (evChain: the same chain, a few
// operations either side) reports the time it ADDED: from its start, or from the latest end of another launch of the chain that lies inside its interval,
// to its own end.  Launches that finish one after the other in the order they were enqueued thus report end(k) - end(k - 1), a launch nothing overlapped
// reports exactly its interval, and the figures of a loop are disjoint pieces of its wall time whatever the order the launches finished in.
float timedMs(tbvh_context* c, uint64_t seq) {
    constexpr uint64_t R = tbvh_context::kTimeRing;
    const uint32_t slot = (uint32_t)(seq % R);
    float own = -1.0f;
    if (hipEventElapsedTime(&own, c->evRing[slot][0], c->evRing[slot][1]) != hipSuccess) { (void)hipGetLastError(); return -1.0f; }
    const uint32_t chain = c->evChain[slot];
    if (!chain) return own;
    // Launches that ran at the same time were enqueued near each other: a launch starts after the launches before it on its own lane have ended and, of those
    // on the other lane, all but the last overlapDepth - 1 have started (LaneBook::gate) — beside a launch ran at most the other lane's last kMaxDepth launches
    // before it and the launches that lane took until the next one of this lane.  Alternating lanes that is 2 x kMaxDepth numbers either side; a lane takes
    // several launches in a row only for buffers that conflict there, which the book holds kMaxInFlight of before it joins.
    constexpr uint64_t kReach = 2 * LaneBook::kMaxInFlight * LaneBook::kMaxDepth;
    const uint64_t oldest = c->evSeq > R ? c->evSeq - R : 0;
    const uint64_t lo = seq > oldest + kReach ? seq - kReach : oldest, hi = seq + kReach < c->evSeq ? seq + kReach + 1 : c->evSeq;
    float from = 0.f;   // ms after this launch's start
    for (uint64_t j = lo; j < hi; j++) {
        const uint32_t sj = (uint32_t)(j % R);
        if (j == seq || c->evChain[sj] != chain || !c->evDone[sj]) continue;
        float endJ = 0.f;
        if (hipEventSynchronize(c->evRing[sj][1]) != hipSuccess || hipEventElapsedTime(&endJ, c->evRing[slot][0], c->evRing[sj][1]) != hipSuccess) { (void)hipGetLastError(); continue; }
        const bool before = endJ < own || (endJ == own && j < seq);   // (equal time stamps: in the order enqueued)
        if (before && endJ > from) from = endJ;
    }
    return own - from;
}
}  // namespace tbvh_capi

extern "C" {

int tbvh_abi_version(void) { return TBVH_ABI_VERSION; }
const char* tbvh_last_error(void) { return g_err; }

int tbvh_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { fail(TBVH_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e)); return e == hipErrorNoDevice ? 0 : TBVH_E_HIP; }
    return n;
}

int tbvh_init(int device, tbvh_context** out) {
    if (!out) return fail(TBVH_E_INVALID, "tbvh_init: out is null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(TBVH_E_NODEVICE, "no HIP device available");
    if (device < 0 || device >= n) return fail(TBVH_E_NODEVICE, "device %d out of range (0..%d)", device, n - 1);
    tbvh_context* c = new (std::nothrow) tbvh_context;
    if (!c) return fail(TBVH_E_NOMEM, "out of host memory");
    c->device = device;
    hipDeviceProp_t prop;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->ownStream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(TBVH_E_HIP, "context setup failed: %s", hipGetErrorString(e)); }
    c->stream = c->ownStream;
    c->numCUs = prop.multiProcessorCount;
    // persistent grid: one-wave workgroups, enough to fill every SIMD several times over
    c->blocks = (uint32_t)c->numCUs * 24u;
    if (const char* e = getenv("TBVH_BLOCKS_PER_CU")) {  // experiment knob
        const int b = atoi(e);
        if (b >= 1 && b <= 32) { c->blocks = (uint32_t)c->numCUs * (uint32_t)b; c->gridOverride = true; }
    }
    if (const char* e = getenv("TBVH_RAYS_PER_BLOCK")) {  // experiment knob
        const int b = atoi(e);
        if (b >= 64 && b <= 4096) { c->raysPerBlock = (uint32_t)b; c->gridOverride = true; }
    }
    if (const char* e = getenv("TBVH_SPLIT_RAYS")) { if (atoi(e) == 0) c->splitBelow = 0; }
    if (const char* e = getenv("TBVH_INCOHERENT_COPIES")) { if (atoi(e) == 0) c->incoherentCopies = false; }
    if (const char* e = getenv("TBVH_EMBED_TRIS")) { if (atoi(e) == 0) c->embedTris = false; }
    if (const char* e = getenv("TBVH_DEBUG_FLAGS")) c->expFlags = (uint32_t)strtoul(e, nullptr, 0);   // tbvh_debug_set_flags from the environment (counter runs of tools/)
    if (const char* e = getenv("TBVH_COHERENT_TUNER")) { const int v = atoi(e); c->cohTunerMode = v == 0 ? 1 : (v == 2 ? 2 : (v == 3 ? 3 : 0)); }   // 0: off (always deferred + gated), 2: always strict, 3: always one traversal per wave
    if (const char* e = getenv("TBVH_OVERLAP")) { if (atoi(e) == 0) c->overlap = false; }   // every launch on lane 0 (tbvh_context_set_overlap)
    if (const char* e = getenv("TBVH_OVERLAP_DEPTH")) { const int v = atoi(e); if (v >= 1 && v <= LaneBook::kMaxDepth) c->overlapDepth = v; }   // launches one lane may start ahead of the other (tbvh_debug_set_overlap_depth)
    if (const char* e = getenv("TBVH_PROBE_MEMORY")) { if (atoi(e) == 0) c->probeMemoryOn = false; }   // every probed launch is two flavors (tbvh_debug_set_probe_memory)
    if (const char* e = getenv("TBVH_POOL_PARTS")) {  // experiment knob
        const int b = atoi(e);
        if (b >= 0 && (1 << b) <= kPoolParts) c->poolParts = (uint32_t)b;   // log2 of the partition count
    }
    c->spillEntries = 232;  // 32-bit entries per lane beyond the LDS part of the stack
    if (const char* e2 = getenv("TBVH_SPILL_ENTRIES")) {   // a SMALLER spill area: how the tests reach the "traversal stack overflow" path with a tree of a few hundred levels
        const int v = atoi(e2);
        if (v >= 2 && v <= 232) c->spillEntries = (uint32_t)v & ~1u;
    }
    const size_t spillBytes = (size_t)(c->blocks + c->blocks / 3u) * 64 * c->spillEntries * 4;   // the largest grid any launch uses
    e = c->spill.alloc(spillBytes / 4);
    if (e == hipSuccess) e = c->counter.alloc(32);
    if (e == hipSuccess) e = c->pool.alloc((size_t)(kPoolParts + 1) * kPoolCounterStride * 2);
    if (e != hipSuccess) { tbvh_shutdown(c); return fail(TBVH_E_NOMEM, "device allocation failed: %s", hipGetErrorString(e)); }
    c->status = (uint32_t*)(c->counter.get() + 4);
    hipMemset(c->counter, 0, 256);
    *out = c;
    return 0;
}

void tbvh_shutdown(tbvh_context* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->lane1.stream) hipStreamSynchronize(c->lane1.stream);
    if (c->ownStream) hipStreamSynchronize(c->ownStream);
    c->lane1Dirty = false;
    for (;;) {   // TLASes first: they hold references to their BLASes
        tbvh_scene* t = nullptr;
        for (tbvh_scene* s : c->scenes) if (s->isTlas) { t = s; break; }
        if (!t) break;
        tbvh_free_scene(t);
    }
    while (!c->scenes.empty()) tbvh_free_scene(c->scenes.back());
    freePosesOf(c);
    freeGraphsOf(c);
    freeViewersOf(c);
    freeShadingsOf(c);
    freeOmmStagingOf(c);
    for (const tbvh_context::PinnedRange& r : c->pinned) hipHostFree(r.host);   // (memory of tbvh_pinned_malloc the caller never gave back goes with the context)
    c->pinned.clear();
    delete c->pipe;
    for (auto& pair : c->evRing) for (hipEvent_t ev : pair) if (ev) hipEventDestroy(ev);
    if (c->evBase) hipEventDestroy(c->evBase);
    if (c->probeSlots) hipHostFree(c->probeSlots);   // (both lanes were idle above: no kernel still stores a verdict)
    if (c->lane1.stream) hipStreamDestroy(c->lane1.stream);
    if (c->ownStream) hipStreamDestroy(c->ownStream);
    delete c;   // (its device buffers go here: the device is current, its stream was idle)
}

int tbvh_debug_device_allocations(uint64_t out[2]) {
    if (!out) return fail(TBVH_E_INVALID, "tbvh_debug_device_allocations: null argument");
    out[0] = g_devBufLive.load(); out[1] = g_devBufBytes.load();
    return 0;
}

int tbvh_debug_lbvh_topology(const uint64_t* keys, uint64_t n, int keyBits, uint32_t* out4) {
    if (!keys || !out4 || n < 2 || n > 0x7fffffffull || (keyBits != 32 && keyBits != 64))
        return fail(TBVH_E_INVALID, "tbvh_debug_lbvh_topology: null argument, n = %llu (2 .. 2^31 - 1) or key_bits = %d (32 or 64)", (unsigned long long)n, keyBits);
    std::vector<uint32_t> k32;
    if (keyBits == 32) k32.assign(keys, keys + n);   // (the low words)
    for (int i = 0; i < (int)n - 1; i++) {
        const lbvh::KarrasNode k = keyBits == 32 ? lbvh::karras_node(k32.data(), (int)n, i) : lbvh::karras_node(keys, (int)n, i);
        out4[4 * (size_t)i] = k.left; out4[4 * (size_t)i + 1] = k.right; out4[4 * (size_t)i + 2] = k.lo; out4[4 * (size_t)i + 3] = k.hi;
    }
    return 0;
}

int tbvh_debug_lbvh_ordered(const double* values, uint64_t n, int bits, uint64_t* encoded, double* decoded) {
    if ((n && (!values || !encoded || !decoded)) || (bits != 32 && bits != 64)) return fail(TBVH_E_INVALID, "tbvh_debug_lbvh_ordered: null argument or bits = %d (32 or 64)", bits);
    for (uint64_t i = 0; i < n; i++) {
        if (bits == 32) { const uint32_t e = lbvh::ordered_encode((float)values[i]); encoded[i] = e; decoded[i] = lbvh::ordered_decode(e); }
        else { encoded[i] = lbvh::ordered_encode(values[i]); decoded[i] = lbvh::ordered_decode(encoded[i]); }
    }
    return 0;
}

int tbvh_debug_build_scratch_bytes(uint32_t n, uint64_t sortTemp, uint64_t scanTemp, uint64_t out[6]) {
    if (!out) return fail(TBVH_E_INVALID, "tbvh_debug_build_scratch_bytes: null argument");
    out[0] = lbvh_scratch_total(n, sortTemp); out[1] = ploc_scratch_total(n, sortTemp, scanTemp);
    out[2] = tlas_build_scratch_total(n, sortTemp); out[3] = tlas_dbl_build_scratch_total(n, sortTemp);
    out[4] = sah_scratch_total(n, sortTemp, scanTemp); out[5] = sbvh_scratch_total(n, scanTemp);
    return 0;
}

int tbvh_synchronize(tbvh_context* c) {
    if (!c) return fail(TBVH_E_INVALID, "null context");
    TBVH_ENTER(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int tbvh_set_stream(tbvh_context* c, void* s) {
    if (!c) return fail(TBVH_E_INVALID, "null context");
    TBVH_ENTER(c);   // (lane 1 is used on the context's own stream only: what it holds is joined into that stream before the context leaves it)
    c->stream = s ? (hipStream_t)s : c->ownStream;
    return 0;
}

int tbvh_context_set_overlap(tbvh_context* c, int enabled) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_context_set_overlap: null context");
    TBVH_ENTER(c);
    c->overlap = enabled != 0;
    return 0;
}

// The lane rule of overlap_lanes.h driven by a script, without a device (tests/test_overlap_lanes_host.py).  The book the script works on is the type the
// contexts keep; a launch's slot is its row number.
int tbvh_debug_lane_script(const uint64_t* ops5, uint64_t nOps, int32_t* out) {
    if ((!ops5 || !out) && nOps) return fail(TBVH_E_INVALID, "tbvh_debug_lane_script: null argument");
    LaneBook book;
    std::vector<uint8_t> done(nOps, 0);
    bool allowLane1 = true;
    auto prune = [&] { book.prune([&](int, uint32_t slot) { return done[slot] != 0; }); };
    for (uint64_t i = 0; i < nOps; i++) {
        const uint64_t* op = ops5 + i * 5;
        out[i] = 0;
        switch (op[0]) {
        case 0: {
            LaneFootprint fp;
            fp.rays.lo = (uintptr_t)op[1]; fp.rays.hi = (uintptr_t)op[2]; fp.occ.lo = (uintptr_t)op[3]; fp.occ.hi = (uintptr_t)op[4];
            prune();
            const LaneChoice ch = book.decide(fp, allowLane1);
            if (ch.join) book.joined();
            book.add(ch.lane, fp, (uint32_t)i);
            out[i] = ch.lane + (ch.join ? 2 : 0);
            break;
        }
        case 1:
            if (op[1] >= nOps) return fail(TBVH_E_INVALID, "tbvh_debug_lane_script: row %llu finishes a row beyond the script", (unsigned long long)i);
            done[op[1]] = 1;
            break;
        case 2: allowLane1 = op[1] != 0; break;
        case 3: prune(); out[i] = book.count[0] + 256 * book.count[1]; break;
        default: return fail(TBVH_E_INVALID, "tbvh_debug_lane_script: row %llu has no such operation", (unsigned long long)i);
        }
    }
    return 0;
}

// The same script with the rule for WHEN a launch may start (LaneBook::gate, at the given depth) and the memory of the probe's verdicts (probe_memory.h),
// again without a device (tests/test_lane_runahead_host.py).  Rows of 6 x u64; out: two numbers per row.  Operations 0-3 as above, and for a launch (0)
// out[2 i + 1] = the row of the launch whose start it waits for, or -1;
//   4: an entry point that joins the lanes;
//   5: a probed launch {rays lo, rays hi, scene, any hit, lane}: the finished launches' verdicts are harvested, out[2 i] = 1 if it goes solo; it is remembered;
//   6: what the probe of row op[1] counted: op[2] = 1 incoherent, 2 coherent, 0 nothing (read when that row is seen finished, operation 1).
int tbvh_debug_runahead_script(const uint64_t* ops6, uint64_t nOps, int depth, int64_t* out2) {
    if ((!ops6 || !out2) && nOps) return fail(TBVH_E_INVALID, "tbvh_debug_runahead_script: null argument");
    if (depth < 1 || depth > LaneBook::kMaxDepth) return fail(TBVH_E_INVALID, "tbvh_debug_runahead_script: depth %d (1..%d)", depth, LaneBook::kMaxDepth);
    LaneBook book;
    ProbeMemory memory;
    std::vector<uint8_t> done(nOps, 0), said(nOps, 0);
    bool allowLane1 = true;
    auto prune = [&] { book.prune([&](int, uint32_t slot) { return done[slot] != 0; }); };
    for (uint64_t i = 0; i < nOps; i++) {
        const uint64_t* op = ops6 + i * 6;
        out2[2 * i] = 0; out2[2 * i + 1] = -1;
        if ((op[0] == 1 || op[0] == 6) && op[1] >= nOps) return fail(TBVH_E_INVALID, "tbvh_debug_runahead_script: row %llu names a row beyond the script", (unsigned long long)i);
        switch (op[0]) {
        case 0: {
            LaneFootprint fp;
            fp.rays.lo = (uintptr_t)op[1]; fp.rays.hi = (uintptr_t)op[2]; fp.occ.lo = (uintptr_t)op[3]; fp.occ.hi = (uintptr_t)op[4];
            prune();
            const LaneChoice ch = book.decide(fp, allowLane1);
            if (ch.join) book.joined();
            const uint64_t g = book.gate(ch.lane, depth, [&](uint64_t id) { return done[id] != 0; });
            book.add(ch.lane, fp, (uint32_t)i, i);
            out2[2 * i] = ch.lane + (ch.join ? 2 : 0);
            out2[2 * i + 1] = g == LaneBook::kNoGate ? -1 : (int64_t)g;
            break;
        }
        case 1: done[op[1]] = 1; break;
        case 2: allowLane1 = op[1] != 0; break;
        case 3: prune(); out2[2 * i] = book.count[0] + 256 * book.count[1]; break;
        case 4: book.joined(); break;
        case 5: {
            ProbeKey key;
            key.lo = (uintptr_t)op[1]; key.hi = (uintptr_t)op[2]; key.scene = (const void*)(uintptr_t)op[3]; key.any = op[4] != 0;
            memory.harvest([&](uint64_t id) { return done[id] ? 1 : 0; }, [&](uint64_t id) { return (int)said[id]; });
            out2[2 * i] = memory.solo(key) ? 1 : 0;
            memory.note(key, i, (int)(op[5] & 1u));
            break;
        }
        case 6: said[op[1]] = (uint8_t)(op[2] <= 2 ? op[2] : 0); break;
        default: return fail(TBVH_E_INVALID, "tbvh_debug_runahead_script: row %llu has no such operation", (unsigned long long)i);
        }
    }
    return 0;
}

// What launchQuery plans for a launch (launch_plan.h: the two functions it calls, in its order), from facts stated as words; no device, no scene
// (tests/test_launch_plan_host.py).
int tbvh_debug_launch_plan(const uint64_t* facts, uint32_t nFacts, uint32_t* out, uint32_t nOut) {
    if (!facts || !out) return fail(TBVH_E_INVALID, "tbvh_debug_launch_plan: null argument");
    if (!(nFacts == kLaunchFactWords && nOut == kLaunchPlanWords) && !(nFacts == kLaunchFactWordsTest && nOut == kLaunchPlanWordsTest))   // (as before the triangle test, or with it)
        return fail(TBVH_E_INVALID, "tbvh_debug_launch_plan: %u facts and %u plan words (this library: %u and %u)", nFacts, nOut, kLaunchFactWords,
                    kLaunchPlanWords);
    const LaunchFacts f = launchFactsFromWords(facts, nFacts);
    if (!f.raysPerBlock) return fail(TBVH_E_INVALID, "tbvh_debug_launch_plan: raysPerBlock is 0");
    LaunchPlan p = planBatch(f);
    planShape(p, f);
    launchPlanToWords(p, out, nOut);
    return 0;
}

// What reclassifyTlas plans for a TLAS (tlas_plan.h: the function it calls), from facts stated as words; no device, no scene (tests/test_tlas_plan_host.py).
int tbvh_debug_tlas_plan(const uint64_t* facts, uint32_t nWords, uint32_t* out, uint32_t nOut) {
    if (!facts || !out) return fail(TBVH_E_INVALID, "tbvh_debug_tlas_plan: null argument");
    std::vector<TlasBlasFacts> blas;
    std::vector<TlasView> v0, v1;
    uint32_t at = 0, atOut = 0;
    while (at < nWords) {   // cases back to back, each as long as its BLAS count says
        const uint64_t n = nWords - at >= kTlasFactHead ? facts[at] : ~0ull;
        if (n == 0 || n > nWords - at - kTlasFactHead || n > nOut - atOut || kTlasPlanHead > nOut - atOut - n)
            return fail(TBVH_E_INVALID, "tbvh_debug_tlas_plan: the case at word %u does not fit %u fact words and %u plan words", at, nWords, nOut);
        blas.resize(n); v0.resize(n); v1.resize(n);
        for (uint64_t i = 0; i < n; i++) blas[i] = tlasBlasFactsFromWord(facts[at + kTlasFactHead + i]);
        TlasFacts f;
        f.blas = blas.data(); f.nBlas = (uint32_t)n; f.anyHitSeen = facts[at + 1] != 0; f.hasNodes = facts[at + 2] != 0; f.cap8 = facts[at + 3]; f.cap4 = facts[at + 4];
        TlasView* const view[2] = {v0.data(), v1.data()};
        const TlasPlan p = planTlas(f, view);
        tlasPlanToWords(p, view, f.nBlas, out + atOut);
        at += kTlasFactHead + (uint32_t)n; atOut += kTlasPlanHead + (uint32_t)n;
    }
    if (atOut != nOut) return fail(TBVH_E_INVALID, "tbvh_debug_tlas_plan: %u plan words for cases that fill %u", nOut, atOut);
    return 0;
}

// ... and the facts a live TLAS would state now beside the plan it has stored (tests/test_tlas_plan_gpu.py)
int tbvh_debug_tlas_state(tbvh_scene* s, uint64_t* factsOut, uint32_t* planOut) {
    if (!s || !s->isTlas || s->layout == TBVH_LAYOUT_BVH_DOUBLE || !factsOut || !planOut) return fail(TBVH_E_INVALID, "tbvh_debug_tlas_state: not a TLAS, or a null argument");
    TBVH_LOCK(s->ctx);
    std::vector<TlasBlasFacts> blas;
    const TlasFacts f = tlasFactsNow(s, blas);
    factsOut[0] = f.nBlas; factsOut[1] = f.anyHitSeen; factsOut[2] = f.hasNodes; factsOut[3] = f.cap8; factsOut[4] = f.cap4;
    for (uint32_t i = 0; i < f.nBlas; i++) factsOut[kTlasFactHead + i] = tlasBlasFactsToWord(blas[i]);
    const TlasView* const view[2] = {s->tlas.view[0].data(), s->tlas.view[1].data()};
    tlasPlanToWords(s->tlas.plan, view, f.nBlas, planOut);
    return 0;
}

int tbvh_debug_set_overlap_depth(tbvh_context* c, int depth) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_debug_set_overlap_depth: null context");
    if (depth < 1 || depth > LaneBook::kMaxDepth) return fail(TBVH_E_INVALID, "tbvh_debug_set_overlap_depth: depth %d (1..%d)", depth, LaneBook::kMaxDepth);
    TBVH_ENTER(c);
    c->overlapDepth = depth;
    return 0;
}

int tbvh_debug_set_probe_memory(tbvh_context* c, int enabled) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_debug_set_probe_memory: null context");
    TBVH_ENTER(c);
    c->probeMemoryOn = enabled != 0;
    c->probeMemory.clear();   // (what was learnt under the other setting is not carried over)
    return 0;
}

int tbvh_debug_probe_memory_stats(tbvh_context* c, uint64_t out[2]) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_debug_probe_memory_stats: null argument");
    TBVH_LOCK(c);
    out[0] = c->soloLaunches; out[1] = c->probeVerdicts;
    return 0;
}

// The packet kernel's child filter (packet_cull.h) and its exact per-lane test, both as k_cwbvh_packet runs them for one 64-ray chunk, on the host
// (tests/test_packet_cull_host.py): the same functions, the same order of planes, the same rules for when the filter is off.
int tbvh_debug_packet_cull(const void* nodes80, uint64_t nNodes, const void* rays64, uint64_t haveMask, const float* tcull64, uint8_t* maybeOut, uint8_t* exactOut,
                           uint32_t* chunkFlags) {
    if (!rays64 || !tcull64 || haveMask == 0 || (nNodes && (!nodes80 || !maybeOut || !exactOut)))
        return fail(TBVH_E_INVALID, "tbvh_debug_packet_cull: null argument or no lane holds a ray");
    using namespace tbvh;
    float O[64][3], rD[64][3];
    uint32_t oct[64];
    for (int l = 0; l < 64; l++) {
        const float* r = (const float*)((const uint8_t*)rays64 + 64 * l);
        for (int a = 0; a < 3; a++) { O[l][a] = r[a]; rD[l][a] = r[8 + a]; }
        oct[l] = 7u - ((rD[l][0] < 0 ? 4u : 0u) | (rD[l][1] < 0 ? 2u : 0u) | (rD[l][2] < 0 ? 1u : 0u));
    }
    const int first = __builtin_ctzll(haveMask);
    const uint32_t oct0 = oct[first];
    const bool neg0[3] = {((7u - oct0) & 4u) != 0, ((7u - oct0) & 2u) != 0, ((7u - oct0) & 1u) != 0};
    bool mixed = false, raysFinite = true;
    float Olo[3], Ohi[3], rlo[3], rhi[3], TC = -1.0f;
    for (int a = 0; a < 3; a++) { Olo[a] = Ohi[a] = O[first][a]; rlo[a] = rhi[a] = rD[first][a]; }
    for (int l = 0; l < 64; l++) {
        if (!((haveMask >> l) & 1u)) continue;
        mixed |= oct[l] != oct0;
        for (int a = 0; a < 3; a++) {
            raysFinite &= pkc_finite(O[l][a]) && pkc_finite(rD[l][a]);
            Olo[a] = __builtin_fminf(Olo[a], O[l][a]); Ohi[a] = __builtin_fmaxf(Ohi[a], O[l][a]);
            rlo[a] = __builtin_fminf(rlo[a], rD[l][a]); rhi[a] = __builtin_fmaxf(rhi[a], rD[l][a]);
        }
        TC = __builtin_fmaxf(TC, pk_cull_tc(tcull64[l]));
    }
    const bool useCull = !mixed && raysFinite;
    if (chunkFlags) *chunkFlags = (mixed ? 1u : 0u) | (raysFinite ? 0u : 2u);
    for (uint64_t n = 0; n < nNodes; n++) {
        const uint8_t* node = (const uint8_t*)nodes80 + 80 * n;
        float n0[3];
        uint32_t ew;
        memcpy(n0, node, 12); memcpy(&ew, node + 12, 4);
        const int e[3] = {(int)(int8_t)ew, (int)(int8_t)(ew >> 8), (int)(int8_t)(ew >> 16)};
        const uint8_t* meta = node + 24;
        const uint8_t* qbytes = node + 32;
        float planes[8][6], bounds[8][6];
        bool allFinite = true;
        for (uint32_t L = 0; L < 48; L++) {     // what lane L of the wave does
            const uint32_t p = L >> 3, axis = p % 3u, isHi = p / 3u, dstPlane = axis + 3u * (isHi ^ (neg0[axis] ? 1u : 0u));
            const float qf = (float)qbytes[L];
            planes[L & 7u][dstPlane] = qf;
            bool fin;
            bounds[L & 7u][dstPlane] = pk_cull_plane(dstPlane >= 3u, qf, n0[axis], e[axis], Olo[axis], Ohi[axis], rlo[axis], rhi[axis], fin);
            allFinite &= fin;
        }
        float ax[64][3], ox[64][3];                  // each lane's ldexpf(rD, e) and (n0 - O) * rD, as the kernel forms them
        for (int l = 0; l < 64; l++)
            for (int a = 0; a < 3; a++) { ax[l][a] = ldexpf(rD[l][a], e[a]); ox[l][a] = (n0[a] - O[l][a]) * rD[l][a]; }
        uint32_t maybe = 0, exact = 0;
        for (uint32_t c = 0; c < 8; c++) {
            if (meta[c] == 0) continue;
            const float* b = bounds[c];
            if (!useCull || pk_cull_pass(b[0], b[1], b[2], b[3], b[4], b[5], TC, allFinite)) maybe |= 1u << c;
            const float* q = planes[c];
            for (int l = 0; l < 64 && !((exact >> c) & 1u); l++) {
                if (!((haveMask >> l) & 1u)) continue;
                const bool in = mixed ? pk_child_exact<true>(q[0], q[1], q[2], q[3], q[4], q[5], ax[l][0], ax[l][1], ax[l][2], ox[l][0], ox[l][1], ox[l][2], tcull64[l])
                                      : pk_child_exact<false>(q[0], q[1], q[2], q[3], q[4], q[5], ax[l][0], ax[l][1], ax[l][2], ox[l][0], ox[l][1], ox[l][2], tcull64[l]);
                if (in) exact |= 1u << c;
            }
        }
        maybeOut[n] = (uint8_t)maybe; exactOut[n] = (uint8_t)exact;
    }
    return 0;
}

// The ray / triangle test in its two forms (device_common.h), on the host (tests/test_tri_flat_host.py): tri_test with its early-outs, as the per-lane kernels run
// it, and tri_test_flat, as the wave-packet kernel runs it.  Both are made of the same helpers; the library is built with -ffp-contract=off on the host too.
int tbvh_debug_tri_test_flat(const float* od6, const float* tri9, const float* tmax, uint64_t n, uint8_t* acceptBranch, uint8_t* acceptFlat, float* tuvBranch,
                             float* tuvFlat) {
    if (n && (!od6 || !tri9 || !tmax || !acceptBranch || !acceptFlat || !tuvBranch || !tuvFlat)) return fail(TBVH_E_INVALID, "tbvh_debug_tri_test_flat: null argument");
    for (uint64_t i = 0; i < n; i++) {
        const float* r = od6 + 6 * i;
        const float* t = tri9 + 9 * i;
        const float3 O = make_float3(r[0], r[1], r[2]), D = make_float3(r[3], r[4], r[5]);
        const float3 v0 = make_float3(t[0], t[1], t[2]), e1 = make_float3(t[3], t[4], t[5]), e2 = make_float3(t[6], t[7], t[8]);
        TriHit hb = {0.f, 0.f, 0.f}, hf = {0.f, 0.f, 0.f};
        acceptBranch[i] = tri_test(O, D, v0, e1, e2, tmax[i], hb) ? 1 : 0;
        acceptFlat[i] = tri_test_flat(O, D, v0, e1, e2, tmax[i], hf) ? 1 : 0;
        tuvBranch[3 * i] = hb.t; tuvBranch[3 * i + 1] = hb.u; tuvBranch[3 * i + 2] = hb.v;
        tuvFlat[3 * i] = hf.t; tuvFlat[3 * i + 1] = hf.u; tuvFlat[3 * i + 2] = hf.v;
    }
    return 0;
}

int tbvh_debug_overlap_stats(tbvh_context* c, uint64_t out[2]) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_debug_overlap_stats: null argument");
    TBVH_LOCK(c);
    out[0] = c->lane1Launches; out[1] = c->laneJoins;
    return 0;
}

float tbvh_time_last_ms(tbvh_context* c) {
    if (!c) return -1.0f;
    TBVH_LOCK(c);
    if (!c->timed) return -1.0f;
    if (c->hostQuerySeq == c->evSeq && c->hostQueryMs >= 0.f) return c->hostQueryMs;   // a host-array query runs as several launches: their sum
    hipSetDevice(c->device);
    if (hipEventSynchronize(c->ev1) != hipSuccess) return -1.0f;
    if (c->evSeq && c->ev1 == c->evRing[(c->evSeq - 1) % tbvh_context::kTimeRing][1]) return timedMs(c, c->evSeq - 1);   // (not so: a wavefront frame's own pair)
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) return -1.0f;
    return ms;
}

int tbvh_time_history(tbvh_context* c, float* ms, uint32_t cap, uint32_t* count) {
    if (!c || !count || (!ms && cap)) return fail(TBVH_E_INVALID, "tbvh_time_history: null argument");
    *count = 0;
    TBVH_ENTER(c);
    uint64_t n = c->evSeq < tbvh_context::kTimeRing ? c->evSeq : tbvh_context::kTimeRing;
    if (n > cap) n = cap;
    for (uint64_t i = 0; i < n; i++) {   // oldest first
        const uint32_t slot = (uint32_t)((c->evSeq - n + i) % tbvh_context::kTimeRing);
        float t = -1.0f;
        if (c->evDone[slot]) {
            HIP_TRY(hipEventSynchronize(c->evRing[slot][1]));
            t = timedMs(c, c->evSeq - n + i);
            if (t < 0.f && !c->evChain[slot]) HIP_TRY(hipEventElapsedTime(&t, c->evRing[slot][0], c->evRing[slot][1]));   // (reports the failure)
        }
        ms[i] = t;
    }
    *count = (uint32_t)n;
    return 0;
}

int tbvh_debug_stats(tbvh_context* c, uint64_t out[8], int reset) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_debug_stats: null argument");
    TBVH_ENTER(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->counter + 8, 64, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(c->counter + 8, 0, 64));
    return 0;
}

int tbvh_set_timing(tbvh_context* c, int enabled) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_set_timing: null context");
    TBVH_LOCK(c);
    c->skipTiming = enabled == 0;
    return 0;
}

int tbvh_debug_set_flags(tbvh_context* c, uint32_t flags) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_debug_set_flags: null context");
    TBVH_LOCK(c);
    c->expFlags = flags;
    return 0;
}

int tbvh_debug_last_probe(tbvh_context* c, uint32_t out[3]) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_debug_last_probe: null argument");
    TBVH_ENTER(c);
    out[0] = out[1] = out[2] = 0;
    if (!c->lastProbed) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    // (the area the last launch drew from, on the lane it took: the next launch's kernels will zero it)
    const uint32_t* pool = c->lastProbedLane ? c->lane1.pool.get() : c->pool.get();
    const int last = (c->lastProbedLane ? c->lane1.poolCur : c->poolCur) ^ 1;
    HIP_TRY(hipMemcpy(out, pool + (size_t)last * ((size_t)(kPoolParts + 1) * kPoolCounterStride) + (size_t)kPoolParts * kPoolCounterStride, 8, hipMemcpyDeviceToHost));
    out[2] = (out[1] != 0 && out[0] * 10u >= out[1] * 6u) ? 2u : 1u;   // the rule of k_cwbvh (kernels_cwbvh.hip)
    return 0;
}

// ---- device buffers ------------------------------------------------------------------------

int tbvh_device_malloc(tbvh_context* c, uint64_t bytes, void** out) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_device_malloc: null argument");
    TBVH_ENTER(c);
    hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(TBVH_E_NOMEM, "hipMalloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(e));
    return 0;
}
int tbvh_device_free(tbvh_context* c, void* p) {
    if (!c) return fail(TBVH_E_INVALID, "null context");
    TBVH_ENTER(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipFree(p));
    return 0;
}
int tbvh_copy_to_device(tbvh_context* c, void* d, const void* src, uint64_t bytes) {
    if (!c || ((!d || !src) && bytes)) return fail(TBVH_E_INVALID, "tbvh_copy_to_device: null argument");
    TBVH_ENTER(c);
    HIP_TRY(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}
int tbvh_copy_from_device(tbvh_context* c, void* dst, const void* d, uint64_t bytes) {
    if (!c || ((!d || !dst) && bytes)) return fail(TBVH_E_INVALID, "tbvh_copy_from_device: null argument");
    TBVH_ENTER(c);
    HIP_TRY(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// Device memory bandwidth as this GPU delivers it today: a streaming copy (one float4 per thread, non-temporal; read + written bytes
// counted) and a read-only sweep over `bytes`, best of `reps` launches each.  The denominators of the roofline lines in bench.py.
static int timeBest(tbvh_context* c, uint32_t reps, const std::function<void()>& launch, double* bestMs) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); return fail(TBVH_E_HIP, "hipEventCreate failed"); }
    double best = 0;
    hipError_t err = hipSuccess;
    for (uint32_t i = 0; i <= reps && err == hipSuccess; i++) {   // the first launch warms up
        err = hipEventRecord(e0, c->stream);
        launch();
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipEventRecord(e1, c->stream);
        if (err == hipSuccess) err = hipEventSynchronize(e1);
        float ms = 0;
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
        if (err == hipSuccess && i && ms > 0 && (best == 0 || ms < best)) best = ms;
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    if (err != hipSuccess) return fail(TBVH_E_HIP, "measurement launch failed: %s", hipGetErrorString(err));
    if (best <= 0) return fail(TBVH_E_HIP, "measurement produced no timing");
    *bestMs = best;
    return 0;
}

int tbvh_measure_copy_bandwidth(tbvh_context* c, uint64_t bytes, uint32_t reps, double* gbps) {
    if (!c || !gbps || bytes < (1u << 20)) return fail(TBVH_E_INVALID, "tbvh_measure_copy_bandwidth: null argument or under 1 MB");
    TBVH_ENTER(c);
    DevBuf<void> a, b;
    if (a.alloc(bytes) != hipSuccess || b.alloc(bytes) != hipSuccess) return fail(TBVH_E_NOMEM, "tbvh_measure_copy_bandwidth: cannot allocate 2 x %llu bytes", (unsigned long long)bytes);
    int r = 0;
    if (hipMemsetAsync(a, 1, bytes, c->stream) != hipSuccess) r = fail(TBVH_E_HIP, "hipMemsetAsync failed");
    double ms = 0;
    if (!r) r = timeBest(c, reps ? reps : 3, [&] { launch_stream_copy((const float4*)a.get(), (float4*)b.get(), bytes / 16, c->stream); }, &ms);
    if (r) return r;
    *gbps = 2.0 * (double)bytes / (ms * 1e-3) / 1e9;
    return 0;
}

int tbvh_measure_read_bandwidth(tbvh_context* c, uint64_t bytes, uint32_t reps, double* gbps) {
    if (!c || !gbps || bytes < (1u << 20)) return fail(TBVH_E_INVALID, "tbvh_measure_read_bandwidth: null argument or under 1 MB");
    TBVH_ENTER(c);
    DevBuf<void> a;
    DevBuf<float> sink;
    if (a.alloc(bytes) != hipSuccess || sink.alloc(64) != hipSuccess) return fail(TBVH_E_NOMEM, "tbvh_measure_read_bandwidth: cannot allocate %llu bytes", (unsigned long long)bytes);
    int r = 0;
    if (hipMemsetAsync(a, 1, bytes, c->stream) != hipSuccess) r = fail(TBVH_E_HIP, "hipMemsetAsync failed");
    double ms = 0;
    if (!r) r = timeBest(c, reps ? reps : 3, [&] { launch_stream_read((const float4*)a.get(), sink, bytes / 16, (uint32_t)c->numCUs * 32u, c->stream); }, &ms);
    if (r) return r;
    *gbps = (double)bytes / (ms * 1e-3) / 1e9;
    return 0;
}

// Host link as this box delivers it: one pinned buffer, hipMemcpyAsync up and down, best of `reps` each.  The denominator of bench.py's
// detail.host_rays (a host tinybvh::Ray[] costs 64 bytes up and 20 bytes down per ray).
int tbvh_measure_link_bandwidth(tbvh_context* c, uint64_t bytes, uint32_t reps, double* h2d_gbps, double* d2h_gbps) {
    if (!c || !h2d_gbps || !d2h_gbps || bytes < (1u << 20)) return fail(TBVH_E_INVALID, "tbvh_measure_link_bandwidth: null argument or under 1 MB");
    TBVH_ENTER(c);
    void* h = nullptr;
    DevBuf<void> d;
    if (hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess) return fail(TBVH_E_NOMEM, "tbvh_measure_link_bandwidth: cannot pin %llu bytes", (unsigned long long)bytes);
    if (d.alloc(bytes) != hipSuccess) { hipHostFree(h); return fail(TBVH_E_NOMEM, "tbvh_measure_link_bandwidth: cannot allocate %llu device bytes", (unsigned long long)bytes); }
    memset(h, 1, bytes);
    double up = 0, down = 0;
    int r = timeBest(c, reps ? reps : 3, [&] { (void)hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream); }, &up);
    if (!r) r = timeBest(c, reps ? reps : 3, [&] { (void)hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream); }, &down);
    hipHostFree(h);
    if (r) return r;
    *h2d_gbps = (double)bytes / (up * 1e-3) / 1e9; *d2h_gbps = (double)bytes / (down * 1e-3) / 1e9;
    return 0;
}

// VALU issue ceiling of this GPU for the instruction mix of the CWBVH node test (kernels_raygen.hip: k_valu_mix), 8 waves per SIMD:
// wave64 VALU instructions per second over the whole chip, in units of 1e9.
int tbvh_measure_valu_issue(tbvh_context* c, uint32_t reps, double* ginstr_per_s) {
    if (!c || !ginstr_per_s) return fail(TBVH_E_INVALID, "tbvh_measure_valu_issue: null argument");
    TBVH_ENTER(c);
    const uint32_t blocks = (uint32_t)c->numCUs * 32u;
    const int iters = 20000;
    DevBuf<float> out;
    if (out.alloc((size_t)blocks * 64) != hipSuccess) return fail(TBVH_E_NOMEM, "tbvh_measure_valu_issue: out of device memory");
    double ms = 0;
    const int r = timeBest(c, reps ? reps : 3, [&] { launch_valu_mix(out, iters, blocks, c->stream); }, &ms);
    if (r) return r;
    *ginstr_per_s = (double)blocks * iters * 32.0 / (ms * 1e-3) / 1e9;
    return 0;
}

}  // extern "C"
