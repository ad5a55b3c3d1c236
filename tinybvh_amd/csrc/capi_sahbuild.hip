// capi_sahbuild.hip — the reference's binned-SAH tree as a BVH2 in the caller's memory: built on the device (kernels_sahbuild.hip) or by the
// sequential host twin (sahbuild_host.cpp), both over sah_split.h.  The scene-making forms (tbvh_build_device_sah, tbvh_build_device_mesh with
// builder 2) are in capi_scene.hip beside the other device builders.
#include "capi_internal.h"
#include "sahbuild.h"

using namespace tbvh;
using namespace tbvh_capi;

namespace {
// the output rules both entry points share: the count is always reported; arrays are written only when both fit
int checkOutputs(const char* who, uint64_t need, uint64_t nTris, const void* nodesOut, uint64_t capNodes, const void* idxOut, uint64_t capIdx) {
    if (!nodesOut) return 0;
    if (!idxOut) return fail(TBVH_E_INVALID, "%s: nodes32_out without prim_idx_out", who);
    if (capNodes < need || capIdx < nTris)
        return fail(TBVH_E_INVALID, "%s: %llu nodes and %llu indices do not fit (capacity %llu / %llu)", who, (unsigned long long)need, (unsigned long long)nTris,
                    (unsigned long long)capNodes, (unsigned long long)capIdx);
    return 0;
}
}  // namespace

extern "C" {

int tbvh_host_build_bvh2_sah(const tbvh_mesh* mesh, uint32_t maxLeafTris, void* nodesOut, uint64_t capNodes, uint32_t* idxOut, uint64_t capIdx, uint64_t* nNodesOut) {
    if (!nNodesOut) return fail(TBVH_E_INVALID, "tbvh_host_build_bvh2_sah: null argument");
    if (mesh && mesh->on_device) return fail(TBVH_E_INVALID, "tbvh_host_build_bvh2_sah: the host builder reads host memory (on_device = 0)");
    if (int r = checkMesh(mesh, "tbvh_host_build_bvh2_sah")) return r;
    if (mesh->n_tris > 0x3fffffffull) return fail(TBVH_E_INVALID, "tbvh_host_build_bvh2_sah: too many triangles for 32-bit node indices");
    std::vector<Node2> nodes;
    std::vector<uint32_t> idx;
    try {
        sah_build_host(HostMesh(mesh->verts, mesh->stride_bytes, mesh->indices), (uint32_t)mesh->n_tris, maxLeafTris, nodes, idx);
    } catch (const std::bad_alloc&) { return fail(TBVH_E_NOMEM, "tbvh_host_build_bvh2_sah: out of host memory"); }
    *nNodesOut = nodes.size();
    if (int r = checkOutputs("tbvh_host_build_bvh2_sah", nodes.size(), mesh->n_tris, nodesOut, capNodes, idxOut, capIdx)) return r;
    if (nodesOut) {
        memcpy(nodesOut, nodes.data(), nodes.size() * sizeof(Node2));
        memcpy(idxOut, idx.data(), idx.size() * 4);
    }
    return 0;
}

int tbvh_build_bvh2_sah_device(tbvh_context* c, const tbvh_mesh* mesh, uint32_t maxLeafTris, void* nodesOut, uint64_t capNodes, uint32_t* idxOut, uint64_t capIdx,
                               int outOnDevice, uint64_t* nNodesOut) {
    if (!c || !nNodesOut) return fail(TBVH_E_INVALID, "tbvh_build_bvh2_sah_device: null argument");
    if (int r = checkMesh(mesh, "tbvh_build_bvh2_sah_device")) return r;
    const uint64_t nTris = mesh->n_tris;
    if (nTris > 0x3fffffffull) return fail(TBVH_E_INVALID, "tbvh_build_bvh2_sah_device: too many triangles for 32-bit node indices");
    if (nodesOut && outOnDevice && (((uintptr_t)nodesOut & 15) || ((uintptr_t)idxOut & 3)))
        return fail(TBVH_E_INVALID, "tbvh_build_bvh2_sah_device: device outputs must be 16-byte (nodes) and 4-byte (indices) aligned");
    TBVH_ENTER(c);
    DevBuf<float4> n2;
    DevBuf<uint32_t> idx;
    DevBuf<void> scratch;
    DeviceMesh dm;
    if (int r = stageMesh(c, *mesh, dm)) return r;
    size_t sortTemp = 0, scanTemp = 0;
    const size_t scratchBytes = sah_scratch_bytes((uint32_t)nTris, &sortTemp, &scanTemp);
    HIP_TRY(n2.alloc(nTris * 4)); HIP_TRY(idx.alloc(nTris)); HIP_TRY(scratch.alloc(scratchBytes));
    uint32_t nNodes = 0;
    HIP_TRY(timedBegin(c));
    HIP_TRY(run_sah_build(dm.src, (uint32_t)nTris, maxLeafTris, c->sahSmallSubtree, n2, idx, scratch, sortTemp, scanTemp, c->status, c->stream, &nNodes));
    HIP_TRY(timedEnd(c));
    if (int r = checkStatus(c)) return r;   // (a device-resident index that is not a vertex: TBVH_E_FORMAT)
    *nNodesOut = nNodes;
    if (int r = checkOutputs("tbvh_build_bvh2_sah_device", nNodes, nTris, nodesOut, capNodes, idxOut, capIdx)) return r;
    if (nodesOut) {
        const hipMemcpyKind kind = outOnDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        HIP_TRY(hipMemcpyAsync(nodesOut, n2, (size_t)nNodes * 32, kind, c->stream));
        HIP_TRY(hipMemcpyAsync(idxOut, idx, nTris * 4, kind, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int tbvh_debug_set_sah_small_subtree(tbvh_context* c, uint32_t n) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_debug_set_sah_small_subtree: null argument");
    TBVH_LOCK(c);
    c->sahSmallSubtree = n;
    return 0;
}

}  // extern "C"
