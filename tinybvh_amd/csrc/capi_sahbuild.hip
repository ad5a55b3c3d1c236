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

// the host twin over a box source into the caller's arrays
int hostBoxBuild(const char* who, const SahBoxes& boxes, uint64_t n, uint32_t maxLeaf, void* nodesOut, uint64_t capNodes, uint32_t* idxOut, uint64_t capIdx,
                 uint64_t* nNodesOut) {
    if (!boxes.data || !nNodesOut) return fail(TBVH_E_INVALID, "%s: null argument", who);
    if (n == 0 || n > 0x3fffffffull) return fail(TBVH_E_INVALID, "%s: %llu primitives (1 .. 2^30 - 1)", who, (unsigned long long)n);
    std::vector<Node2> nodes;
    std::vector<uint32_t> idx;
    try {
        sah_build_host(boxes, (uint32_t)n, maxLeaf, nodes, idx);
    } catch (const std::bad_alloc&) { return fail(TBVH_E_NOMEM, "%s: out of host memory", who); }
    *nNodesOut = nodes.size();
    if (int r = checkOutputs(who, nodes.size(), n, nodesOut, capNodes, idxOut, capIdx)) return r;
    if (nodesOut) {
        memcpy(nodesOut, nodes.data(), nodes.size() * sizeof(Node2));
        memcpy(idxOut, idx.data(), idx.size() * 4);
    }
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
    HIP_TRY(run_sah_build(dm.src, (uint32_t)nTris, maxLeafTris, c->sahSmallSubtree, c->sahOneGroup, n2, idx, scratch, sortTemp, scanTemp, c->status, c->stream, &nNodes));
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

int tbvh_host_build_bvh2_sah_aabbs(const void* aabbs32, uint64_t n, uint32_t maxLeaf, void* nodesOut, uint64_t capNodes, uint32_t* idxOut, uint64_t capIdx,
                                   uint64_t* nNodesOut) {
    return hostBoxBuild("tbvh_host_build_bvh2_sah_aabbs", sah_boxes_aabbs(aabbs32), n, maxLeaf, nodesOut, capNodes, idxOut, capIdx, nNodesOut);
}

int tbvh_host_build_bvh2_sah_spheres(const void* spheres16, uint64_t n, uint32_t maxLeaf, void* nodesOut, uint64_t capNodes, uint32_t* idxOut, uint64_t capIdx,
                                     uint64_t* nNodesOut) {
    return hostBoxBuild("tbvh_host_build_bvh2_sah_spheres", sah_boxes_spheres(spheres16), n, maxLeaf, nodesOut, capNodes, idxOut, capIdx, nNodesOut);
}

int tbvh_host_build_tlas_sah(const void* instances192, uint64_t n, void* nodes64Out, uint64_t capNodes, uint32_t* idxOut, uint64_t capIdx, uint64_t* nNodesOut) {
    const char* who = "tbvh_host_build_tlas_sah";
    if (!instances192 || !nNodesOut) return fail(TBVH_E_INVALID, "%s: null argument", who);
    if (n == 0 || n > 0x3fffffffull) return fail(TBVH_E_INVALID, "%s: %llu instances (1 .. 2^30 - 1)", who, (unsigned long long)n);
    BVH2 bvh;
    std::vector<NodeAL> al;
    try {
        sah_build_host(sah_boxes_instances(instances192), (uint32_t)n, 0, bvh.nodes, bvh.primIdx);
        bvh.triCount = (uint32_t)n;
        encode_bvh_gpu(bvh, al);   // (BVH_GPU::ConvertFrom: depth-first pre-order, the pad node 1 not emitted)
    } catch (const std::bad_alloc&) { return fail(TBVH_E_NOMEM, "%s: out of host memory", who); }
    *nNodesOut = al.size();
    if (int r = checkOutputs(who, al.size(), n, nodes64Out, capNodes, idxOut, capIdx)) return r;
    if (nodes64Out) {
        memcpy(nodes64Out, al.data(), al.size() * sizeof(NodeAL));
        memcpy(idxOut, bvh.primIdx.data(), bvh.primIdx.size() * 4);
    }
    return 0;
}

int tbvh_build_bvh2_sah_device_aabbs(tbvh_context* c, const void* aabbs32, uint64_t n, int onDevice, uint32_t maxLeaf, void* nodesOut, uint64_t capNodes,
                                     uint32_t* idxOut, uint64_t capIdx, int outOnDevice, uint64_t* nNodesOut) {
    const char* who = "tbvh_build_bvh2_sah_device_aabbs";
    if (!c || !aabbs32 || !nNodesOut) return fail(TBVH_E_INVALID, "%s: null argument", who);
    if (n == 0 || n > 0x3fffffffull) return fail(TBVH_E_INVALID, "%s: %llu boxes (1 .. 2^30 - 1)", who, (unsigned long long)n);
    if (onDevice && ((uintptr_t)aabbs32 & 3)) return fail(TBVH_E_INVALID, "%s: device boxes must be 4-byte aligned", who);
    if (nodesOut && outOnDevice && (((uintptr_t)nodesOut & 15) || ((uintptr_t)idxOut & 3)))
        return fail(TBVH_E_INVALID, "%s: device outputs must be 16-byte (nodes) and 4-byte (indices) aligned", who);
    TBVH_ENTER(c);
    DevBuf<float4> n2, staged;
    DevBuf<uint32_t> idx;
    DevBuf<void> scratch;
    const void* dBoxes = aabbs32;
    if (!onDevice) {
        HIP_TRY(staged.alloc(n * 2));
        HIP_TRY(hipMemcpyAsync(staged, aabbs32, n * 32, hipMemcpyHostToDevice, c->stream));
        dBoxes = staged.get();
    }
    size_t sortTemp = 0, scanTemp = 0;
    const size_t scratchBytes = sah_scratch_bytes((uint32_t)n, &sortTemp, &scanTemp);
    HIP_TRY(n2.alloc(n * 4)); HIP_TRY(idx.alloc(n)); HIP_TRY(scratch.alloc(scratchBytes));
    uint32_t nNodes = 0;
    HIP_TRY(timedBegin(c));
    HIP_TRY(run_sah_build(SahSrc(sah_boxes_aabbs(dBoxes)), (uint32_t)n, maxLeaf, c->sahSmallSubtree, c->sahOneGroup, n2, idx, scratch, sortTemp, scanTemp, c->status,
                          c->stream, &nNodes));
    HIP_TRY(timedEnd(c));
    *nNodesOut = nNodes;
    if (int r = checkOutputs(who, nNodes, n, nodesOut, capNodes, idxOut, capIdx)) return r;
    if (nodesOut) {
        const hipMemcpyKind kind = outOnDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        HIP_TRY(hipMemcpyAsync(nodesOut, n2, (size_t)nNodes * 32, kind, c->stream));
        HIP_TRY(hipMemcpyAsync(idxOut, idx, n * 4, kind, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int tbvh_debug_set_sah_one_group(tbvh_context* c, uint32_t n) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_debug_set_sah_one_group: null argument");
    TBVH_LOCK(c);
    c->sahOneGroup = n;
    return 0;
}

int tbvh_debug_get_sah_thresholds(tbvh_context* c, uint32_t out[2]) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_debug_get_sah_thresholds: null argument");
    TBVH_LOCK(c);
    out[0] = c->sahSmallSubtree; out[1] = c->sahOneGroup;
    return 0;
}

int tbvh_debug_set_sah_small_subtree(tbvh_context* c, uint32_t n) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_debug_set_sah_small_subtree: null argument");
    TBVH_LOCK(c);
    c->sahSmallSubtree = n;
    return 0;
}

}  // extern "C"
