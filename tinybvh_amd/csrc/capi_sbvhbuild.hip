// capi_sbvhbuild.hip — the reference's spatial-split tree (SBVH, BVH::BuildHQ) as a BVH2 in the caller's memory: built on the device
// (kernels_sbvhbuild.hip) or by the sequential host twin (sbvhbuild_host.cpp), both over sbvh_split.h; and the scene-making forms (that builder, then
// the device conversion).
#include "capi_internal.h"
#include "sbvhbuild.h"

using namespace tbvh;
using namespace tbvh_capi;

namespace {
// the output rules the entry points share: the counts are always reported; arrays are written only when both fit
int checkOutputs(const char* who, uint64_t needNodes, uint64_t needIdx, const void* nodesOut, uint64_t capNodes, const void* idxOut, uint64_t capIdx) {
    if (!nodesOut) return 0;
    if (!idxOut) return fail(TBVH_E_INVALID, "%s: nodes32_out without prim_idx_out", who);
    if (capNodes < needNodes || capIdx < needIdx)
        return fail(TBVH_E_INVALID, "%s: %llu nodes and %llu indices do not fit (capacity %llu / %llu)", who, (unsigned long long)needNodes, (unsigned long long)needIdx,
                    (unsigned long long)capNodes, (unsigned long long)capIdx);
    return 0;
}

void publish(const sbvh::Stats& st, tbvh_sbvh_stats* out) {
    if (!out) return;
    out->n_refs = st.refs; out->n_spatial_splits = st.spatialSplits; out->n_unsplit_left = st.unsplitLeft; out->n_unsplit_right = st.unsplitRight;
    out->n_fragment_splits = st.fragmentSplits; out->n_one_sided_splits = st.oneSidedSplits; out->n_clipped_reclips = st.clippedReclips;
    out->n_budget_refusals = st.budgetRefusals; out->n_failed_partitions = st.failedPartitions;
}

// 3 n + 2 temporary nodes are counted in an int (the scan over them): the most triangles a build takes
constexpr uint64_t kMaxTris = (0x7fffffffull - 2) / 3;

// the device arrays of one build (3 n nodes, n + n / 2 references, the scratch), allocated before the build is timed
struct BuildBuffers {
    DevBuf<float4> n2;
    DevBuf<uint32_t> idx;
    DevBuf<void> scratch;
    size_t scanTemp = 0;
};
int allocBuild(uint64_t nTris, BuildBuffers& b) {
    const size_t scratchBytes = sbvh_scratch_bytes((uint32_t)nTris, &b.scanTemp);
    HIP_TRY(b.n2.alloc((nTris * 3 + 2) * 2)); HIP_TRY(b.idx.alloc(nTris + nTris / 2 + 1)); HIP_TRY(b.scratch.alloc(scratchBytes));
    return 0;
}

int sbvhLeafTris(const char* who, int layout, uint32_t& maxLeafTris) {
    if (layout != TBVH_LAYOUT_CWBVH && layout != TBVH_LAYOUT_BVH4_GPU) return fail(TBVH_E_INVALID, "%s: target layout %d not supported (BVH8_CWBVH and BVH4_GPU are)", who, layout);
    const uint32_t leafCap = layout == TBVH_LAYOUT_CWBVH ? 3u : 4u;
    if (maxLeafTris == 0) maxLeafTris = leafCap;
    if (maxLeafTris > leafCap) return fail(TBVH_E_INVALID, "%s: at most %u triangles per leaf for this layout", who, leafCap);
    return 0;
}

int buildScene(const char* who, tbvh_context* c, const tbvh_mesh& mesh, int layout, uint32_t maxLeafTris, tbvh_scene** out) {
    const uint64_t nTris = mesh.n_tris;
    if (!c || !mesh.verts || !out || nTris == 0) return fail(TBVH_E_INVALID, "%s: null/empty argument", who);
    if (int r = sbvhLeafTris(who, layout, maxLeafTris)) return r;
    if (nTris > kMaxTris) return fail(TBVH_E_INVALID, "%s: too many triangles (at most %llu)", who, (unsigned long long)kMaxTris);
    TBVH_ENTER(c);
    BuildBuffers b;
    DeviceMesh dm;
    if (int r = stageMesh(c, mesh, dm)) return r;
    if (int r = allocBuild(nTris, b)) return r;
    uint32_t nNodes = 0, nIdx = 0;
    HIP_TRY(timedBegin(c));
    HIP_TRY(run_sbvh_build(dm.src, (uint32_t)nTris, maxLeafTris, b.n2, b.idx, b.scratch, b.scanTemp, c->status, c->stream, &nNodes, &nIdx, nullptr));
    b.scratch.reset();
    if (int r = checkStatus(c)) return r;
    int r = convertDeviceImpl(c, layout, b.n2, nNodes, b.idx, nIdx, dm.src, out);
    HIP_TRY(timedEnd(c));
    if (r || !dm.src.indices) return r;
    r = keepMeshIndices(*out, dm.src);
    if (!r && hipStreamSynchronize((*out)->ctx->stream) != hipSuccess) r = fail(TBVH_E_HIP, "%s: copying the index buffer failed", who);
    if (r) { tbvh_free_scene(*out); *out = nullptr; }
    return r;
}
}  // namespace

extern "C" {

int tbvh_host_build_bvh2_sbvh(const tbvh_mesh* mesh, uint32_t maxLeafTris, void* nodesOut, uint64_t capNodes, uint32_t* idxOut, uint64_t capIdx, uint64_t* nNodesOut,
                              uint64_t* nIdxOut, tbvh_sbvh_stats* stats) {
    if (!nNodesOut || !nIdxOut) return fail(TBVH_E_INVALID, "tbvh_host_build_bvh2_sbvh: null argument");
    if (mesh && mesh->on_device) return fail(TBVH_E_INVALID, "tbvh_host_build_bvh2_sbvh: the host builder reads host memory (on_device = 0)");
    if (int r = checkMesh(mesh, "tbvh_host_build_bvh2_sbvh")) return r;
    if (mesh->n_tris > kMaxTris) return fail(TBVH_E_INVALID, "tbvh_host_build_bvh2_sbvh: too many triangles (at most %llu)", (unsigned long long)kMaxTris);
    std::vector<Node2> nodes;
    std::vector<uint32_t> idx;
    sbvh::Stats st;
    try {
        sbvh_build_host(HostMesh(mesh->verts, mesh->stride_bytes, mesh->indices), (uint32_t)mesh->n_tris, maxLeafTris, nodes, idx, &st);
    } catch (const std::bad_alloc&) { return fail(TBVH_E_NOMEM, "tbvh_host_build_bvh2_sbvh: out of host memory"); }
    *nNodesOut = nodes.size(); *nIdxOut = idx.size();
    publish(st, stats);
    if (int r = checkOutputs("tbvh_host_build_bvh2_sbvh", nodes.size(), idx.size(), nodesOut, capNodes, idxOut, capIdx)) return r;
    if (nodesOut) {
        memcpy(nodesOut, nodes.data(), nodes.size() * sizeof(Node2));
        memcpy(idxOut, idx.data(), idx.size() * 4);
    }
    return 0;
}

int tbvh_build_bvh2_sbvh_device(tbvh_context* c, const tbvh_mesh* mesh, uint32_t maxLeafTris, void* nodesOut, uint64_t capNodes, uint32_t* idxOut, uint64_t capIdx,
                                int outOnDevice, uint64_t* nNodesOut, uint64_t* nIdxOut, tbvh_sbvh_stats* stats) {
    if (!c || !nNodesOut || !nIdxOut) return fail(TBVH_E_INVALID, "tbvh_build_bvh2_sbvh_device: null argument");
    if (int r = checkMesh(mesh, "tbvh_build_bvh2_sbvh_device")) return r;
    const uint64_t nTris = mesh->n_tris;
    if (nTris > kMaxTris) return fail(TBVH_E_INVALID, "tbvh_build_bvh2_sbvh_device: too many triangles (at most %llu)", (unsigned long long)kMaxTris);
    if (nodesOut && outOnDevice && (((uintptr_t)nodesOut & 15) || ((uintptr_t)idxOut & 3)))
        return fail(TBVH_E_INVALID, "tbvh_build_bvh2_sbvh_device: device outputs must be 16-byte (nodes) and 4-byte (indices) aligned");
    TBVH_ENTER(c);
    BuildBuffers b;
    DeviceMesh dm;
    if (int r = stageMesh(c, *mesh, dm)) return r;
    if (int r = allocBuild(nTris, b)) return r;
    uint32_t nNodes = 0, nIdx = 0;
    sbvh::Stats st;
    HIP_TRY(timedBegin(c));
    HIP_TRY(run_sbvh_build(dm.src, (uint32_t)nTris, maxLeafTris, b.n2, b.idx, b.scratch, b.scanTemp, c->status, c->stream, &nNodes, &nIdx, &st));
    HIP_TRY(timedEnd(c));
    if (int r = checkStatus(c)) return r;   // (a device-resident index that is not a vertex: TBVH_E_FORMAT)
    *nNodesOut = nNodes; *nIdxOut = nIdx;
    publish(st, stats);
    if (int r = checkOutputs("tbvh_build_bvh2_sbvh_device", nNodes, nIdx, nodesOut, capNodes, idxOut, capIdx)) return r;
    if (nodesOut) {
        const hipMemcpyKind kind = outOnDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        HIP_TRY(hipMemcpyAsync(nodesOut, b.n2, (size_t)nNodes * 32, kind, c->stream));
        HIP_TRY(hipMemcpyAsync(idxOut, b.idx, (size_t)nIdx * 4, kind, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int tbvh_build_device_sbvh(tbvh_context* c, const void* verts16, uint64_t nTris, int onDevice, int layout, uint32_t maxLeafTris, tbvh_scene** out) {
    return buildScene("tbvh_build_device_sbvh", c, flatMesh(verts16, nTris, onDevice), layout, maxLeafTris, out);
}

int tbvh_build_device_sbvh_mesh(tbvh_context* c, const tbvh_mesh* mesh, int layout, uint32_t maxLeafTris, tbvh_scene** out) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_build_device_sbvh_mesh: null argument");
    if (int r = checkMesh(mesh, "tbvh_build_device_sbvh_mesh")) return r;
    return buildScene("tbvh_build_device_sbvh_mesh", c, *mesh, layout, maxLeafTris, out);
}

}  // extern "C"
