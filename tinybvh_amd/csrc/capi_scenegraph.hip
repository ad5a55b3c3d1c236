// capi_scenegraph.hip — the animated scene graph on the device (tbvh_scenegraph_*; include/tinybvh_amd.h, DESIGN.md par. 17): Scene::UpdateSceneGraph of
// tiny_scene.h without the BLAS and TLAS builds.  A graph is validated and compiled on the host (scenegraph_host.cpp: sg_compile, shared with the host
// twin), goes up once as ONE allocation, and from then on a frame sends one float: the kernels of kernels_scenegraph.hip keep the channels' (t, k), the
// nodes' T, R, S and matrices and the outputs (instance transforms, joint matrices, morph weights) where tbvh_rebuild_tlas_device and tbvh_pose_set_* read
// them.  Two arrays of combined transforms take turns, so that a joint the walk reaches after its mesh node finds last walk's matrix (see the header).
#include "capi_internal.h"
#include "scenegraph_host.h"
#include "../../include/tinybvh_amd_debug.h"

using namespace tbvh;
using namespace tbvh_capi;

struct tbvh_scenegraph {
    tbvh_context* ctx = nullptr;
    SgCompiled c;            // the tables as they went up (counts, offsets, the time limit; the state arrays in it are the initial ones)
    DevBuf<char> mem;        // every array of the graph, 256-byte aligned sections
    SgView view;             // pointers into mem
    float* combinedBuf[2] = {nullptr, nullptr};
    int cur = 0;             // combinedBuf[cur] holds the last walk's result
};

namespace {

struct Packer {
    std::vector<char> bytes;
    template <class T>
    size_t put(const std::vector<T>& v, size_t minCount = 1) {   // (an empty array still gets a section: no null pointers in the view)
        const size_t at = (bytes.size() + 255) & ~(size_t)255;
        bytes.resize(at + std::max(v.size(), minCount) * sizeof(T), 0);
        if (!v.empty()) memcpy(bytes.data() + at, v.data(), v.size() * sizeof(T));
        return at;
    }
};

void setCombined(tbvh_scenegraph* g) {
    g->view.combined = g->combinedBuf[g->cur];
    g->view.combinedPrev = g->combinedBuf[g->cur ^ 1];
}

void walk(tbvh_scenegraph* g) {
    g->cur ^= 1;   // (this walk overwrites every entry of what was the walk before last)
    setCombined(g);
    launch_graph_walk(g->view, -1, g->ctx->stream);
}

}  // namespace

namespace tbvh_capi {
void freeGraphsOf(tbvh_context* c) {
    for (tbvh_scenegraph* g : c->graphs) delete g;
    c->graphs.clear();
}
}  // namespace tbvh_capi

extern "C" {

int tbvh_scenegraph_create(tbvh_context* c, const tbvh_scenegraph_desc* desc, tbvh_scenegraph** out) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_scenegraph_create: null argument");
    tbvh_scenegraph* g = new (std::nothrow) tbvh_scenegraph;
    if (!g) return fail(TBVH_E_NOMEM, "tbvh_scenegraph_create: out of host memory");
    if (int r = sg_compile(desc, "tbvh_scenegraph_create", g->c)) { delete g; return r; }   // (before anything is allocated)
    TBVH_ENTER(c);
    g->ctx = c;
    SgCompiled& h = g->c;
    Packer p;
    const std::vector<float> instOut((size_t)h.nInstances * 16, 0.f), jointOut((size_t)h.nPairs * 16, 0.f);
    const size_t oInterp = p.put(h.sInterp), oType = p.put(h.sType), oKeyOff = p.put(h.sKeyOff), oValOff = p.put(h.sValOff), oTimes = p.put(h.times), oValues = p.put(h.values);
    const size_t oSampler = p.put(h.cSampler), oNode = p.put(h.cNode), oTarget = p.put(h.cTarget), oFlags = p.put(h.cFlags), oT = p.put(h.cT), oK = p.put(h.cK), oTrig = p.put(h.cTrig);
    const size_t oWOff = p.put(h.wOff), oTrs = p.put(h.trs), oWeights = p.put(h.weights), oWritten = p.put(h.written), oMatrix = p.put(h.matrix), oLocal = p.put(h.local);
    const size_t oComb0 = p.put(h.combined), oComb1 = p.put(h.combinedPrev), oAncOff = p.put(h.ancOff), oAnc = p.put(h.anc);
    const size_t oInstNode = p.put(h.instNode), oInstOut = p.put(instOut), oPairMesh = p.put(h.pairMesh), oPairJoint = p.put(h.pairJoint), oPairStale = p.put(h.pairStale);
    const size_t oInvBind = p.put(h.invBind), oJointOut = p.put(jointOut);
    if (g->mem.alloc(p.bytes.size()) != hipSuccess) {
        (void)hipGetLastError();
        delete g;
        return fail(TBVH_E_NOMEM, "tbvh_scenegraph_create: %llu bytes of device memory", (unsigned long long)p.bytes.size());
    }
    if (hipMemcpyAsync(g->mem, p.bytes.data(), p.bytes.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
        delete g;
        return fail(TBVH_E_HIP, "tbvh_scenegraph_create: copying the graph failed: %s", hipGetErrorString(hipGetLastError()));
    }
    char* b = g->mem.get();
    SgView& v = g->view;
    v.nNodes = h.nNodes; v.nSamplers = h.nSamplers; v.nChannels = h.nChannels; v.nInstances = h.nInstances; v.nPairs = h.nPairs;
    v.nTimes = (uint32_t)h.times.size(); v.nValues = (uint32_t)h.values.size(); v.nWeights = (uint32_t)h.weights.size(); v.nAnc = (uint32_t)h.anc.size();
    v.sInterp = (uint32_t*)(b + oInterp); v.sType = (uint32_t*)(b + oType); v.sKeyOff = (uint32_t*)(b + oKeyOff); v.sValOff = (uint32_t*)(b + oValOff);
    v.times = (float*)(b + oTimes); v.values = (float*)(b + oValues);
    v.cSampler = (uint32_t*)(b + oSampler); v.cNode = (uint32_t*)(b + oNode); v.cTarget = (uint32_t*)(b + oTarget); v.cFlags = (uint32_t*)(b + oFlags);
    v.cT = (float*)(b + oT); v.cK = (int32_t*)(b + oK); v.cTrig = (uint32_t*)(b + oTrig);
    v.wOff = (uint32_t*)(b + oWOff); v.trs = (float*)(b + oTrs); v.weights = (float*)(b + oWeights); v.written = (uint32_t*)(b + oWritten);
    v.matrix = (float*)(b + oMatrix); v.local = (float*)(b + oLocal);
    g->combinedBuf[0] = (float*)(b + oComb0); g->combinedBuf[1] = (float*)(b + oComb1);
    v.ancOff = (uint32_t*)(b + oAncOff); v.anc = (uint32_t*)(b + oAnc);
    v.instNode = (uint32_t*)(b + oInstNode); v.instOut = (float*)(b + oInstOut);
    v.pairMesh = (uint32_t*)(b + oPairMesh); v.pairJoint = (uint32_t*)(b + oPairJoint); v.pairStale = (uint32_t*)(b + oPairStale);
    v.invBind = (float*)(b + oInvBind); v.jointOut = (float*)(b + oJointOut);
    v.status = c->status;
    setCombined(g);
    c->graphs.push_back(g);
    *out = g;
    return 0;
}

int tbvh_scenegraph_advance(tbvh_scenegraph* g, float dt) {
    if (!g) return fail(TBVH_E_INVALID, "tbvh_scenegraph_advance: null argument");
    if (int r = sg_check_time(g->c, "tbvh_scenegraph_advance", dt)) return r;
    tbvh_context* c = g->ctx;
    TBVH_ENTER(c);
    HIP_TRY(timedBegin(c));
    launch_graph_sample(g->view, 0, g->c.nChannels, dt, kSgShadowAll, c->stream);
    walk(g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    return 0;
}

int tbvh_scenegraph_advance_animation(tbvh_scenegraph* g, uint32_t a, float dt) {
    if (!g) return fail(TBVH_E_INVALID, "tbvh_scenegraph_advance_animation: null argument");
    if (a >= g->c.nAnimations) return fail(TBVH_E_INVALID, "tbvh_scenegraph_advance_animation: animation %u of %u", a, g->c.nAnimations);
    if (int r = sg_check_time(g->c, "tbvh_scenegraph_advance_animation", dt)) return r;
    tbvh_context* c = g->ctx;
    TBVH_ENTER(c);
    HIP_TRY(timedBegin(c));
    launch_graph_sample(g->view, g->c.animOff[a], g->c.animOff[a + 1], dt, kSgShadowAnim, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    return 0;
}

int tbvh_scenegraph_update_nodes(tbvh_scenegraph* g) {
    if (!g) return fail(TBVH_E_INVALID, "tbvh_scenegraph_update_nodes: null argument");
    tbvh_context* c = g->ctx;
    TBVH_ENTER(c);
    HIP_TRY(timedBegin(c));
    walk(g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    return 0;
}

int tbvh_scenegraph_set_time(tbvh_scenegraph* g, uint32_t a, float t) {
    if (!g) return fail(TBVH_E_INVALID, "tbvh_scenegraph_set_time: null argument");
    if (a >= g->c.nAnimations) return fail(TBVH_E_INVALID, "tbvh_scenegraph_set_time: animation %u of %u", a, g->c.nAnimations);
    if (int r = sg_check_time(g->c, "tbvh_scenegraph_set_time", t)) return r;
    tbvh_context* c = g->ctx;
    TBVH_ENTER(c);
    launch_graph_set_time(g->view.cT, g->view.cK, g->c.animOff[a], g->c.animOff[a + 1], t, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int tbvh_scenegraph_reset(tbvh_scenegraph* g, uint32_t a) {
    if (!g) return fail(TBVH_E_INVALID, "tbvh_scenegraph_reset: null argument");
    return tbvh_scenegraph_set_time(g, a, 0.f);
}

int tbvh_scenegraph_set_local(tbvh_scenegraph* g, uint32_t node, const float* mat16) {
    if (!g || !mat16) return fail(TBVH_E_INVALID, "tbvh_scenegraph_set_local: null argument");
    if (node >= g->c.nNodes) return fail(TBVH_E_INVALID, "tbvh_scenegraph_set_local: node %u of %u", node, g->c.nNodes);
    tbvh_context* c = g->ctx;
    TBVH_ENTER(c);
    SgMat m;
    memcpy(m.m, mat16, 64);
    launch_graph_set_local(g->view.local, node, m, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int tbvh_scenegraph_instance_transforms(tbvh_scenegraph* g, const float** dMats16, uint64_t* n) {
    if (!g || !dMats16) return fail(TBVH_E_INVALID, "tbvh_scenegraph_instance_transforms: null argument");
    *dMats16 = g->view.instOut;
    if (n) *n = g->c.nInstances;
    return 0;
}

int tbvh_scenegraph_joint_matrices(tbvh_scenegraph* g, uint32_t use, const float** dMats16, uint32_t* n) {
    if (!g || !dMats16) return fail(TBVH_E_INVALID, "tbvh_scenegraph_joint_matrices: null argument");
    if (use >= g->c.nUses) return fail(TBVH_E_INVALID, "tbvh_scenegraph_joint_matrices: skin use %u of %u", use, g->c.nUses);
    *dMats16 = g->view.jointOut + (size_t)g->c.useOff[use] * 16;
    if (n) *n = g->c.useOff[use + 1] - g->c.useOff[use];
    return 0;
}

int tbvh_scenegraph_morph_weights(tbvh_scenegraph* g, uint32_t node, const float** dWeights, uint32_t* n) {
    if (!g || !dWeights) return fail(TBVH_E_INVALID, "tbvh_scenegraph_morph_weights: null argument");
    if (node >= g->c.nNodes) return fail(TBVH_E_INVALID, "tbvh_scenegraph_morph_weights: node %u of %u", node, g->c.nNodes);
    *dWeights = g->view.weights + g->c.wOff[node];
    if (n) *n = g->c.wOff[node + 1] - g->c.wOff[node];
    return 0;
}

namespace {
const void* arrayOf(const tbvh_scenegraph* g, int what) {
    const SgView& v = g->view;
    switch (what) {
    case TBVH_GRAPH_TRS: return v.trs;
    case TBVH_GRAPH_LOCAL: return v.local;
    case TBVH_GRAPH_COMBINED: return g->combinedBuf[g->cur];
    case TBVH_GRAPH_CHANNEL_T: return v.cT;
    case TBVH_GRAPH_CHANNEL_K: return v.cK;
    case TBVH_GRAPH_INSTANCES: return v.instOut;
    case TBVH_GRAPH_JOINTS: return v.jointOut;
    case TBVH_GRAPH_WEIGHTS: return v.weights;
    case TBVH_GRAPH_STALE: return v.pairStale;
    case TBVH_GRAPH_TRIG: return v.cTrig;
    }
    return nullptr;
}
}  // namespace

int tbvh_debug_scenegraph_array(tbvh_scenegraph* g, int what, void** dPtr) {
    if (!g || !dPtr) return fail(TBVH_E_INVALID, "tbvh_debug_scenegraph_array: null argument");
    if (!(*dPtr = const_cast<void*>(arrayOf(g, what)))) return fail(TBVH_E_INVALID, "tbvh_debug_scenegraph_array: what = %d", what);
    return 0;
}

int tbvh_debug_scenegraph_step(tbvh_scenegraph* g, int step, float dt) {
    if (!g || step < 0 || step > 3) return fail(TBVH_E_INVALID, "tbvh_debug_scenegraph_step: null graph or step %d", step);
    if (int r = sg_check_time(g->c, "tbvh_debug_scenegraph_step", dt)) return r;
    tbvh_context* c = g->ctx;
    TBVH_ENTER(c);
    HIP_TRY(timedBegin(c));
    if (step == 0) launch_graph_sample(g->view, 0, g->c.nChannels, dt, kSgShadowAll, c->stream);
    else {
        if (step == 2) { g->cur ^= 1; setCombined(g); }
        launch_graph_walk(g->view, step, c->stream);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    return 0;
}

int tbvh_scenegraph_download(tbvh_scenegraph* g, int what, void* dst, uint64_t cap) {
    if (!g || !dst) return fail(TBVH_E_INVALID, "tbvh_scenegraph_download: null argument");
    const void* src = arrayOf(g, what);
    if (!src) return fail(TBVH_E_INVALID, "tbvh_scenegraph_download: what = %d", what);
    const uint64_t bytes = sg_download_bytes(g->c, what);
    if (cap < bytes) return fail(TBVH_E_INVALID, "tbvh_scenegraph_download: room for %llu bytes, %llu needed", (unsigned long long)cap, (unsigned long long)bytes);
    tbvh_context* c = g->ctx;
    TBVH_ENTER(c);
    if (bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return checkStatus(c);   // (synchronizes)
}

void tbvh_scenegraph_free(tbvh_scenegraph* g) {
    if (!g) return;
    tbvh_context* c = g->ctx;
    TBVH_LOCK(c);
    (void)tbvh_capi::setDevice(c);   // (joins the launch lanes)
    hipStreamSynchronize(c->stream);   // (kernels in flight, and the TLAS rebuilds and poses fed from the outputs, read the graph's memory)
    for (size_t i = 0; i < c->graphs.size(); i++)
        if (c->graphs[i] == g) { c->graphs.erase(c->graphs.begin() + i); break; }
    delete g;
}

}  // extern "C"
