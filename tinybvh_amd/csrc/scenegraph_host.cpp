// scenegraph_host.cpp — a scene graph descriptor validated and compiled into scenegraph.h's flat arrays (sg_compile: shared with capi_scenegraph.hip), and
// the host twin tbvh_host_scenegraph_*: scenegraph.h's work items looped over on the CPU.  Plain C++ that needs scenegraph.h, the public header and the
// library's error helper only, so that it can also be compiled on its own (with a sanitizer, into a stand-alone program that supplies tbvh_capi::fail:
// tools/scenegraph_sanitize.cpp).  Built -ffp-contract=off like the rest.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "scenegraph_host.h"
#include "../../include/tinybvh_amd_debug.h"

namespace tbvh_capi {
int fail(int code, const char* fmt, ...);   // (capi_context.hip) sets tbvh_last_error() of the calling thread, returns code
}
using tbvh_capi::fail;

namespace tbvh {

namespace {
typedef unsigned long long ull;
const char* const kTargetName[4] = {"translation", "rotation", "scale", "weights"};

// floats of key_values sampler s must hold to serve a channel with `count` weights (count is ignored unless the sampler holds floats): the largest
// position Sample* can form with k <= keys - 2, plus one
uint64_t neededValues(uint32_t type, uint32_t interp, uint64_t keys, uint64_t count) {
    if (type == TBVH_GRAPH_FLOAT) {
        if (keys == 1) return 1;
        if (interp == TBVH_GRAPH_SPLINE) return std::max<uint64_t>(((keys - 1) * count + count - 1) * 3 + 2, 2);
        if (interp == TBVH_GRAPH_STEP) return keys - 1;
        return (keys - 1) * count + count;
    }
    const uint64_t W = type == TBVH_GRAPH_QUAT ? 4 : 3;
    if (keys == 1) return W;
    if (interp == TBVH_GRAPH_SPLINE) return ((keys - 1) * 3 + 2) * W;
    return keys * W;
}
}  // namespace

int sg_compile(const tbvh_scenegraph_desc* d, const char* who, SgCompiled& g) {
    if (!d) return fail(TBVH_E_INVALID, "%s: null descriptor", who);
    if (d->flags & ~TBVH_SCENEGRAPH_FRESH_JOINTS) return fail(TBVH_E_INVALID, "%s: unknown flags 0x%x", who, d->flags);
    if (d->n_nodes == 0) return fail(TBVH_E_INVALID, "%s: no nodes", who);
    if ((d->n_nodes | d->n_samplers | d->n_animations | d->n_channels | d->n_instances | d->n_skin_uses) >> 32)
        return fail(TBVH_E_INVALID, "%s: a count beyond 32 bits (%llu nodes, %llu samplers, %llu animations, %llu channels, %llu instances, %llu skin uses)", who, (ull)d->n_nodes,
                    (ull)d->n_samplers, (ull)d->n_animations, (ull)d->n_channels, (ull)d->n_instances, (ull)d->n_skin_uses);
    if (!d->parent || !d->translation || !d->rotation || !d->scale || !d->matrix || !d->local_transform) return fail(TBVH_E_INVALID, "%s: a null node array", who);
    if (d->n_samplers && (!d->sampler_interpolation || !d->sampler_type || !d->sampler_key_offset || !d->sampler_value_offset || !d->key_times || !d->key_values))
        return fail(TBVH_E_INVALID, "%s: a null sampler array", who);
    if (d->n_channels && (!d->channel_animation || !d->channel_sampler || !d->channel_node || !d->channel_target)) return fail(TBVH_E_INVALID, "%s: a null channel array", who);
    if (d->n_instances && !d->node_of_instance) return fail(TBVH_E_INVALID, "%s: null node_of_instance", who);
    if (d->n_skin_uses && (!d->skin_mesh_node || !d->skin_joint_offset || !d->skin_joint_node || !d->skin_inverse_bind)) return fail(TBVH_E_INVALID, "%s: a null skin array", who);
    const void* const arrays[] = {d->parent, d->visit_order, d->translation, d->rotation, d->scale, d->matrix, d->local_transform, d->n_weights, d->weights, d->sampler_interpolation,
                                  d->sampler_type, d->sampler_key_offset, d->sampler_value_offset, d->key_times, d->key_values, d->channel_animation, d->channel_sampler,
                                  d->channel_node, d->channel_target, d->node_of_instance, d->skin_mesh_node, d->skin_joint_offset, d->skin_joint_node, d->skin_inverse_bind};
    for (const void* a : arrays)
        if ((uintptr_t)a & 3) return fail(TBVH_E_INVALID, "%s: a misaligned array (4 bytes)", who);
    const uint32_t N = (uint32_t)d->n_nodes, NS = (uint32_t)d->n_samplers, NC = (uint32_t)d->n_channels, NI = (uint32_t)d->n_instances, NU = (uint32_t)d->n_skin_uses;
    if (NC && d->n_animations == 0) return fail(TBVH_E_INVALID, "%s: %u channels and no animation", who, NC);

    // ---- the tree: parents, cycles, the visit order ------------------------------------------------------------------------------------------
    for (uint32_t n = 0; n < N; n++)
        if (d->parent[n] < -1 || d->parent[n] >= (int64_t)N) return fail(TBVH_E_FORMAT, "%s: node %u: parent %d is not a node (%u nodes)", who, n, d->parent[n], N);
    std::vector<uint32_t> depth(N, 0);   // 0 = unknown; a root has 1
    {
        std::vector<uint32_t> path;
        for (uint32_t n = 0; n < N; n++) {
            if (depth[n]) continue;
            path.clear();
            uint32_t a = n;
            while (!depth[a] && d->parent[a] >= 0 && path.size() <= N) { path.push_back(a); a = (uint32_t)d->parent[a]; }
            if (path.size() > N) return fail(TBVH_E_FORMAT, "%s: node %u: its parents form a cycle", who, n);
            if (!depth[a]) depth[a] = 1;   // (a root)
            uint32_t dep = depth[a];
            for (size_t i = path.size(); i-- > 0;) depth[path[i]] = ++dep;
        }
    }
    std::vector<uint32_t> order(N), pre(N), last(N);
    if (d->visit_order) {
        std::vector<uint8_t> seen(N, 0);
        for (uint32_t i = 0; i < N; i++) {
            const uint32_t n = d->visit_order[i];
            if (n >= N || seen[n]) return fail(TBVH_E_FORMAT, "%s: visit_order[%u] = %u is not a node or is listed twice", who, i, n);
            if (d->parent[n] >= 0 && !seen[d->parent[n]]) return fail(TBVH_E_FORMAT, "%s: visit_order[%u]: node %u comes before its parent %d", who, i, n, d->parent[n]);
            seen[n] = 1; order[i] = n; pre[n] = i;
        }
    } else {
        std::vector<uint32_t> childOff(N + 2, 0), child(N);   // children by increasing index, the roots as children of slot N
        for (uint32_t n = 0; n < N; n++) childOff[(d->parent[n] < 0 ? N : (uint32_t)d->parent[n]) + 1]++;
        for (uint32_t n = 0; n <= N; n++) childOff[n + 1] += childOff[n];
        std::vector<uint32_t> fill(childOff.begin(), childOff.end() - 1);
        for (uint32_t n = 0; n < N; n++) child[fill[d->parent[n] < 0 ? N : (uint32_t)d->parent[n]]++] = n;
        std::vector<uint32_t> stack;
        for (uint32_t i = childOff[N + 1]; i-- > childOff[N];) stack.push_back(child[i]);
        uint32_t at = 0;
        while (!stack.empty()) {
            const uint32_t n = stack.back(); stack.pop_back();
            pre[n] = at; order[at++] = n;
            for (uint32_t i = childOff[n + 1]; i-- > childOff[n];) stack.push_back(child[i]);
        }
    }
    {   // the last visit of each subtree; a listing in which a subtree is not one run is no pre-order
        std::vector<uint32_t> size(N, 1);
        for (uint32_t n = 0; n < N; n++) last[n] = pre[n];
        for (uint32_t i = N; i-- > 0;) {
            const uint32_t n = order[i];
            if (d->parent[n] >= 0) { const uint32_t p = (uint32_t)d->parent[n]; size[p] += size[n]; last[p] = std::max(last[p], last[n]); }
        }
        for (uint32_t n = 0; n < N; n++)
            if (last[n] - pre[n] + 1 != size[n]) return fail(TBVH_E_FORMAT, "%s: visit_order is not a depth-first order: the subtree of node %u is not one run", who, n);
    }
    uint64_t nAnc = 0;
    for (uint32_t n = 0; n < N; n++) nAnc += depth[n];
    if (nAnc >> 28) return fail(TBVH_E_INVALID, "%s: the nodes' depths add up to %llu: the ancestor lists are limited to 2^28 entries", who, (ull)nAnc);

    // ---- weights, samplers, channels, instances, skins ------------------------------------------------------------------------------------------
    uint64_t nW = 0;
    if (d->n_weights) for (uint32_t n = 0; n < N; n++) nW += d->n_weights[n];
    if (nW >> 32) return fail(TBVH_E_INVALID, "%s: %llu morph weights", who, (ull)nW);
    float minDur = INFINITY;
    for (uint32_t s = 0; s < NS; s++) {
        const uint32_t k0 = d->sampler_key_offset[s], k1 = d->sampler_key_offset[s + 1], v0 = d->sampler_value_offset[s], v1 = d->sampler_value_offset[s + 1];
        if (d->sampler_interpolation[s] > TBVH_GRAPH_STEP) return fail(TBVH_E_FORMAT, "%s: sampler %u: interpolation %u", who, s, d->sampler_interpolation[s]);
        if (d->sampler_type[s] > TBVH_GRAPH_FLOAT) return fail(TBVH_E_FORMAT, "%s: sampler %u: type %u", who, s, d->sampler_type[s]);
        if (k1 < k0 || v1 < v0) return fail(TBVH_E_FORMAT, "%s: sampler %u: its offsets decrease", who, s);
        if (k1 == k0) return fail(TBVH_E_FORMAT, "%s: sampler %u has no keys", who, s);
        for (uint32_t k = k0; k < k1; k++) {
            const float t = d->key_times[k];
            if (!isfinite(t) || (k > k0 && t < d->key_times[k - 1])) return fail(TBVH_E_FORMAT, "%s: sampler %u: key time %u (%g) is not finite or decreases", who, s, k - k0, (double)t);
        }
        if (d->sampler_type[s] != TBVH_GRAPH_FLOAT) {
            const uint64_t need = neededValues(d->sampler_type[s], d->sampler_interpolation[s], k1 - k0, 0);
            if (v1 - v0 < need) return fail(TBVH_E_FORMAT, "%s: sampler %u: %u key values, %llu needed for %u keys", who, s, v1 - v0, (ull)need, k1 - k0);
        }
        const float dur = d->key_times[k1 - 1];
        if (dur > 0 && k1 - k0 > 1) minDur = std::min(minDur, dur);
        else if (dur < 0 && k1 - k0 > 1) return fail(TBVH_E_FORMAT, "%s: sampler %u: its last key time (%g) is negative", who, s, (double)dur);
    }
    for (uint32_t c = 0; c < NC; c++) {
        const uint32_t a = d->channel_animation[c], s = d->channel_sampler[c], n = d->channel_node[c], t = d->channel_target[c];
        if (a >= d->n_animations || (c && a < d->channel_animation[c - 1])) return fail(TBVH_E_FORMAT, "%s: channel %u: animation %u is not one (%llu) or the channels are not sorted by animation", who, c, a, (ull)d->n_animations);
        if (s >= NS) return fail(TBVH_E_FORMAT, "%s: channel %u: sampler %u is not a sampler (%u)", who, c, s, NS);
        if (n >= N) return fail(TBVH_E_FORMAT, "%s: channel %u: node %u is not a node (%u)", who, c, n, N);
        if (t > 3) return fail(TBVH_E_FORMAT, "%s: channel %u: target %u", who, c, t);
        const uint32_t want = t == 1 ? TBVH_GRAPH_QUAT : t == 3 ? TBVH_GRAPH_FLOAT : TBVH_GRAPH_VEC3;
        if (d->sampler_type[s] != want) return fail(TBVH_E_FORMAT, "%s: channel %u: a %s channel on sampler %u of type %u", who, c, kTargetName[t], s, d->sampler_type[s]);
        if (t == 3) {
            const uint32_t count = d->n_weights ? d->n_weights[n] : 0;
            if (!count) return fail(TBVH_E_FORMAT, "%s: channel %u: a weights channel on node %u, which has no weights", who, c, n);
            const uint64_t have = d->sampler_value_offset[s + 1] - d->sampler_value_offset[s], keys = d->sampler_key_offset[s + 1] - d->sampler_key_offset[s];
            const uint64_t need = neededValues(TBVH_GRAPH_FLOAT, d->sampler_interpolation[s], keys, count);
            if (have < need) return fail(TBVH_E_FORMAT, "%s: channel %u: sampler %u has %llu key values, %llu needed for %llu keys and %u weights", who, c, s, (ull)have, (ull)need, (ull)keys, count);
        }
    }
    for (uint32_t i = 0; i < NI; i++)
        if (d->node_of_instance[i] >= N) return fail(TBVH_E_FORMAT, "%s: instance %u: node %u is not a node (%u)", who, i, d->node_of_instance[i], N);
    for (uint32_t u = 0; u < NU; u++) {
        const uint32_t j0 = d->skin_joint_offset[u], j1 = d->skin_joint_offset[u + 1];
        if (d->skin_mesh_node[u] >= N) return fail(TBVH_E_FORMAT, "%s: skin use %u: mesh node %u is not a node (%u)", who, u, d->skin_mesh_node[u], N);
        if (j1 < j0 || (u == 0 && j0 != 0)) return fail(TBVH_E_FORMAT, "%s: skin use %u: its joint offsets decrease or do not start at 0", who, u);
        if (j1 == j0) return fail(TBVH_E_FORMAT, "%s: skin use %u has no joints", who, u);
        for (uint32_t j = j0; j < j1; j++)
            if (d->skin_joint_node[j] >= N) return fail(TBVH_E_FORMAT, "%s: skin use %u: joint %u: node %u is not a node (%u)", who, u, j - j0, d->skin_joint_node[j], N);
    }

    // ---- everything is in order: the arrays ------------------------------------------------------------------------------------------
    try {
        g = SgCompiled();
        g.nNodes = N; g.nSamplers = NS; g.nChannels = NC; g.nInstances = NI; g.nUses = NU; g.nAnimations = (uint32_t)d->n_animations;
        const uint32_t nTimes = NS ? d->sampler_key_offset[NS] : 0, nValues = NS ? d->sampler_value_offset[NS] : 0;
        g.sInterp.assign(d->sampler_interpolation, d->sampler_interpolation + NS); g.sType.assign(d->sampler_type, d->sampler_type + NS);
        if (NS) { g.sKeyOff.assign(d->sampler_key_offset, d->sampler_key_offset + NS + 1); g.sValOff.assign(d->sampler_value_offset, d->sampler_value_offset + NS + 1); }
        else { g.sKeyOff.assign(1, 0); g.sValOff.assign(1, 0); }
        g.times.assign(d->key_times, d->key_times + nTimes); g.values.assign(d->key_values, d->key_values + nValues);
        g.cSampler.assign(d->channel_sampler, d->channel_sampler + NC); g.cNode.assign(d->channel_node, d->channel_node + NC);
        g.cTarget.assign(d->channel_target, d->channel_target + NC);
        g.cFlags.assign(NC, 0); g.cTrig.assign(NC, 0); g.cT.assign(NC, 0.f); g.cK.assign(NC, 0);
        g.animOff.assign(g.nAnimations + 1, 0);
        for (uint32_t c = 0; c < NC; c++) g.animOff[d->channel_animation[c] + 1]++;
        for (uint32_t a = 0; a < g.nAnimations; a++) g.animOff[a + 1] += g.animOff[a];
        {   // a channel is shadowed when a later one writes the same (node, field): the last writer per field, walking backwards
            std::vector<uint32_t> lastAll((size_t)N * 4, 0xffffffffu);   // the animation of the last writer seen so far (from the end)
            std::vector<uint8_t> any((size_t)N * 4, 0);
            for (uint32_t c = NC; c-- > 0;) {
                const size_t f = (size_t)g.cNode[c] * 4 + g.cTarget[c];
                if (any[f]) g.cFlags[c] |= kSgShadowAll;
                if (any[f] && lastAll[f] == d->channel_animation[c]) g.cFlags[c] |= kSgShadowAnim;
                any[f] = 1; lastAll[f] = d->channel_animation[c];   // (channels are sorted by animation: the nearest later writer decides "same animation")
            }
        }
        g.wOff.assign(N + 1, 0);
        for (uint32_t n = 0; n < N; n++) g.wOff[n + 1] = g.wOff[n] + (d->n_weights ? d->n_weights[n] : 0);
        g.weights.assign((size_t)nW, 0.f);
        if (d->weights && nW) memcpy(g.weights.data(), d->weights, (size_t)nW * 4);
        g.written.assign(N, 0);
        g.trs.resize((size_t)N * 10);
        for (uint32_t n = 0; n < N; n++) {
            float* t = &g.trs[(size_t)n * 10];
            memcpy(t, d->translation + 3 * (size_t)n, 12); memcpy(t + 3, d->rotation + 4 * (size_t)n, 16); memcpy(t + 7, d->scale + 3 * (size_t)n, 12);
        }
        g.matrix.assign(d->matrix, d->matrix + (size_t)N * 16); g.local.assign(d->local_transform, d->local_transform + (size_t)N * 16);
        g.combined.resize((size_t)N * 16);
        for (uint32_t n = 0; n < N; n++) sg_identity(&g.combined[(size_t)n * 16]);
        g.combinedPrev = g.combined;
        g.ancOff.assign(N + 1, 0);
        for (uint32_t n = 0; n < N; n++) g.ancOff[n + 1] = g.ancOff[n] + depth[n];
        g.anc.resize((size_t)nAnc);
        for (uint32_t n = 0; n < N; n++) {
            uint32_t a = n;
            for (uint32_t i = g.ancOff[n + 1]; i-- > g.ancOff[n];) { g.anc[i] = a; a = (uint32_t)d->parent[a]; }
        }
        g.walkOrder = order; g.parent.assign(d->parent, d->parent + N);
        g.instNode.assign(d->node_of_instance, d->node_of_instance + NI);
        g.useOff.assign(1, 0);
        if (NU) g.useOff.assign(d->skin_joint_offset, d->skin_joint_offset + NU + 1);
        g.nPairs = g.useOff[NU];
        if (((uint64_t)g.nPairs + NI) >> 32) return fail(TBVH_E_INVALID, "%s: %u instances and %u joints: together beyond 32 bits", who, NI, g.nPairs);
        g.pairMesh.resize(g.nPairs); g.pairJoint.resize(g.nPairs); g.pairStale.resize(g.nPairs);
        for (uint32_t u = 0; u < NU; u++)
            for (uint32_t p = g.useOff[u]; p < g.useOff[u + 1]; p++) {
                const uint32_t m = d->skin_mesh_node[u], j = d->skin_joint_node[p];
                g.pairMesh[p] = m; g.pairJoint[p] = j;
                g.pairStale[p] = !(d->flags & TBVH_SCENEGRAPH_FRESH_JOINTS) && pre[j] > last[m];
            }
        g.invBind.assign(d->skin_inverse_bind, d->skin_inverse_bind + (size_t)g.nPairs * 16);
        g.maxTime = minDur == INFINITY ? INFINITY : minDur * (float)kSgWrapLimit;
    } catch (const std::bad_alloc&) {
        return fail(TBVH_E_NOMEM, "%s: out of host memory", who);
    }
    return 0;
}

int sg_check_time(const SgCompiled& g, const char* who, float v) {
    if (v != v) return 0;
    if (isinf(v) || fabsf(v) > g.maxTime)
        return fail(TBVH_E_INVALID, "%s: a time of %g: the reference's wrap loop ( while (t >= duration) t -= duration ) would not end or take more than %u turns (limit %g for this graph)", who,
                    (double)v, kSgWrapLimit, (double)g.maxTime);
    return 0;
}

uint64_t sg_download_bytes(const SgCompiled& g, int what) {
    switch (what) {
    case TBVH_GRAPH_TRS: return (uint64_t)g.nNodes * 40;
    case TBVH_GRAPH_LOCAL: case TBVH_GRAPH_COMBINED: return (uint64_t)g.nNodes * 64;
    case TBVH_GRAPH_CHANNEL_T: case TBVH_GRAPH_CHANNEL_K: return (uint64_t)g.nChannels * 4;
    case TBVH_GRAPH_INSTANCES: return (uint64_t)g.nInstances * 64;
    case TBVH_GRAPH_JOINTS: return (uint64_t)g.nPairs * 64;
    case TBVH_GRAPH_WEIGHTS: return (uint64_t)g.weights.size() * 4;
    case TBVH_GRAPH_STALE: return (uint64_t)g.nPairs * 4;
    case TBVH_GRAPH_TRIG: return (uint64_t)g.nChannels * 4;
    }
    return 0;
}

}  // namespace tbvh

using namespace tbvh;

struct tbvh_host_scenegraph {
    SgCompiled c;
    std::vector<float> instOut, jointOut;
    uint32_t status = 0;
};

namespace {

SgView viewOf(tbvh_host_scenegraph* h) {
    SgCompiled& c = h->c;
    SgView v;
    v.nNodes = c.nNodes; v.nSamplers = c.nSamplers; v.nChannels = c.nChannels; v.nInstances = c.nInstances; v.nPairs = c.nPairs;
    v.nTimes = (uint32_t)c.times.size(); v.nValues = (uint32_t)c.values.size(); v.nWeights = (uint32_t)c.weights.size(); v.nAnc = (uint32_t)c.anc.size();
    v.sInterp = c.sInterp.data(); v.sType = c.sType.data(); v.sKeyOff = c.sKeyOff.data(); v.sValOff = c.sValOff.data(); v.times = c.times.data(); v.values = c.values.data();
    v.cSampler = c.cSampler.data(); v.cNode = c.cNode.data(); v.cTarget = c.cTarget.data(); v.cFlags = c.cFlags.data(); v.cT = c.cT.data(); v.cK = c.cK.data(); v.cTrig = c.cTrig.data();
    v.wOff = c.wOff.data(); v.trs = c.trs.data(); v.weights = c.weights.data(); v.written = c.written.data(); v.matrix = c.matrix.data(); v.local = c.local.data();
    v.combined = c.combined.data(); v.combinedPrev = c.combinedPrev.data(); v.ancOff = c.ancOff.data(); v.anc = c.anc.data();
    v.instNode = c.instNode.data(); v.instOut = h->instOut.data(); v.pairMesh = c.pairMesh.data(); v.pairJoint = c.pairJoint.data(); v.pairStale = c.pairStale.data();
    v.invBind = c.invBind.data(); v.jointOut = h->jointOut.data(); v.status = &h->status;
    return v;
}

int report(tbvh_host_scenegraph* h, const char* who) {
    if (!h->status) return 0;
    h->status = 0;
    return fail(TBVH_E_FORMAT, "%s: a sampler, node, key state or key position of the graph was out of range; that item was not written", who);
}

void sample(tbvh_host_scenegraph* h, uint32_t c0, uint32_t c1, float dt, uint32_t mask) {
    const SgView v = viewOf(h);
    for (uint32_t c = c0; c < c1; c++) sg_channel(v, c, dt, mask);
}

void walk(tbvh_host_scenegraph* h) {
    h->c.combined.swap(h->c.combinedPrev);   // (this walk overwrites every entry of what was the walk before last)
    const SgView v = viewOf(h);
    for (uint32_t n = 0; n < v.nNodes; n++) sg_node_local(v, n);
    // combined[n] = combined[parent] * local[n] in visit order: the product sg_node_combine forms down a node's own chain, left to right, without repeating
    // the ancestors' part for every descendant (one thread has no use for the independence a lane per node buys) — the same operations, the same bits
    float ident[16];
    sg_identity(ident);
    for (uint32_t n : h->c.walkOrder) sg_mul(h->c.parent[n] < 0 ? ident : v.combined + 16 * (size_t)h->c.parent[n], v.local + 16 * (size_t)n, v.combined + 16 * (size_t)n);
    for (uint32_t i = 0; i < v.nInstances; i++) sg_instance(v, i);
    for (uint32_t p = 0; p < v.nPairs; p++) sg_joint_pair(v, p);
}

}  // namespace

extern "C" {

int tbvh_host_scenegraph_create(const tbvh_scenegraph_desc* desc, tbvh_host_scenegraph** out) {
    if (!out) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_create: null argument");
    tbvh_host_scenegraph* h = new (std::nothrow) tbvh_host_scenegraph;
    if (!h) return fail(TBVH_E_NOMEM, "tbvh_host_scenegraph_create: out of host memory");
    if (int r = sg_compile(desc, "tbvh_host_scenegraph_create", h->c)) { delete h; return r; }
    h->instOut.assign((size_t)h->c.nInstances * 16, 0.f);
    h->jointOut.assign((size_t)h->c.nPairs * 16, 0.f);
    *out = h;
    return 0;
}

int tbvh_host_scenegraph_advance(tbvh_host_scenegraph* h, float dt) {
    if (!h) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_advance: null argument");
    if (int r = sg_check_time(h->c, "tbvh_host_scenegraph_advance", dt)) return r;
    sample(h, 0, h->c.nChannels, dt, kSgShadowAll);
    walk(h);
    return report(h, "tbvh_host_scenegraph_advance");
}

int tbvh_host_scenegraph_advance_animation(tbvh_host_scenegraph* h, uint32_t a, float dt) {
    if (!h) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_advance_animation: null argument");
    if (a >= h->c.nAnimations) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_advance_animation: animation %u of %u", a, h->c.nAnimations);
    if (int r = sg_check_time(h->c, "tbvh_host_scenegraph_advance_animation", dt)) return r;
    sample(h, h->c.animOff[a], h->c.animOff[a + 1], dt, kSgShadowAnim);
    return report(h, "tbvh_host_scenegraph_advance_animation");
}

int tbvh_host_scenegraph_update_nodes(tbvh_host_scenegraph* h) {
    if (!h) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_update_nodes: null argument");
    walk(h);
    return report(h, "tbvh_host_scenegraph_update_nodes");
}

int tbvh_host_scenegraph_set_time(tbvh_host_scenegraph* h, uint32_t a, float t) {
    if (!h) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_set_time: null argument");
    if (a >= h->c.nAnimations) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_set_time: animation %u of %u", a, h->c.nAnimations);
    if (int r = sg_check_time(h->c, "tbvh_host_scenegraph_set_time", t)) return r;
    for (uint32_t c = h->c.animOff[a]; c < h->c.animOff[a + 1]; c++) { h->c.cT[c] = t; h->c.cK[c] = 0; }
    return 0;
}

int tbvh_host_scenegraph_reset(tbvh_host_scenegraph* h, uint32_t a) { return tbvh_host_scenegraph_set_time(h, a, 0.f); }

int tbvh_host_scenegraph_set_local(tbvh_host_scenegraph* h, uint32_t node, const float* mat16) {
    if (!h || !mat16) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_set_local: null argument");
    if (node >= h->c.nNodes) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_set_local: node %u of %u", node, h->c.nNodes);
    memcpy(&h->c.local[(size_t)node * 16], mat16, 64);
    return 0;
}

int tbvh_debug_host_scenegraph_set_trs(tbvh_host_scenegraph* h, const float* trs10, uint64_t nNodes) {
    if (!h || !trs10) return fail(TBVH_E_INVALID, "tbvh_debug_host_scenegraph_set_trs: null argument");
    if (nNodes != h->c.nNodes) return fail(TBVH_E_INVALID, "tbvh_debug_host_scenegraph_set_trs: %llu nodes, the graph has %u", (unsigned long long)nNodes, h->c.nNodes);
    memcpy(h->c.trs.data(), trs10, h->c.trs.size() * 4);
    return 0;
}

int tbvh_debug_host_scenegraph_check_chains(tbvh_host_scenegraph* h, uint64_t* nDiffer) {
    if (!h || !nDiffer) return fail(TBVH_E_INVALID, "tbvh_debug_host_scenegraph_check_chains: null argument");
    const std::vector<float> walked = h->c.combined;
    const SgView v = viewOf(h);
    for (uint32_t n = 0; n < v.nNodes; n++) sg_node_combine(v, n);
    *nDiffer = 0;
    for (uint32_t n = 0; n < v.nNodes; n++) *nDiffer += memcmp(&walked[(size_t)n * 16], &h->c.combined[(size_t)n * 16], 64) != 0;
    h->c.combined = walked;
    return report(h, "tbvh_debug_host_scenegraph_check_chains");
}

int tbvh_host_scenegraph_instance_transforms(tbvh_host_scenegraph* h, const float** mats16, uint64_t* n) {
    if (!h || !mats16) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_instance_transforms: null argument");
    *mats16 = h->instOut.data();
    if (n) *n = h->c.nInstances;
    return 0;
}

int tbvh_host_scenegraph_joint_matrices(tbvh_host_scenegraph* h, uint32_t use, const float** mats16, uint32_t* n) {
    if (!h || !mats16) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_joint_matrices: null argument");
    if (use >= h->c.nUses) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_joint_matrices: skin use %u of %u", use, h->c.nUses);
    *mats16 = h->jointOut.data() + (size_t)h->c.useOff[use] * 16;
    if (n) *n = h->c.useOff[use + 1] - h->c.useOff[use];
    return 0;
}

int tbvh_host_scenegraph_morph_weights(tbvh_host_scenegraph* h, uint32_t node, const float** weights, uint32_t* n) {
    if (!h || !weights) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_morph_weights: null argument");
    if (node >= h->c.nNodes) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_morph_weights: node %u of %u", node, h->c.nNodes);
    *weights = h->c.weights.data() + h->c.wOff[node];
    if (n) *n = h->c.wOff[node + 1] - h->c.wOff[node];
    return 0;
}

int tbvh_host_scenegraph_download(tbvh_host_scenegraph* h, int what, void* dst, uint64_t cap) {
    if (!h || !dst) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_download: null argument");
    const void* src = nullptr;
    switch (what) {
    case TBVH_GRAPH_TRS: src = h->c.trs.data(); break;
    case TBVH_GRAPH_LOCAL: src = h->c.local.data(); break;
    case TBVH_GRAPH_COMBINED: src = h->c.combined.data(); break;
    case TBVH_GRAPH_CHANNEL_T: src = h->c.cT.data(); break;
    case TBVH_GRAPH_CHANNEL_K: src = h->c.cK.data(); break;
    case TBVH_GRAPH_INSTANCES: src = h->instOut.data(); break;
    case TBVH_GRAPH_JOINTS: src = h->jointOut.data(); break;
    case TBVH_GRAPH_WEIGHTS: src = h->c.weights.data(); break;
    case TBVH_GRAPH_STALE: src = h->c.pairStale.data(); break;
    case TBVH_GRAPH_TRIG: src = h->c.cTrig.data(); break;
    default: return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_download: what = %d", what);
    }
    const uint64_t bytes = sg_download_bytes(h->c, what);
    if (cap < bytes) return fail(TBVH_E_INVALID, "tbvh_host_scenegraph_download: room for %llu bytes, %llu needed", (unsigned long long)cap, (unsigned long long)bytes);
    if (bytes) memcpy(dst, src, bytes);
    return report(h, "tbvh_host_scenegraph_download");
}

void tbvh_host_scenegraph_free(tbvh_host_scenegraph* h) { delete h; }

}  // extern "C"
