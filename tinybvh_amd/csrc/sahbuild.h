// sahbuild.h — the reference's binned-SAH tree (BVH::Build, tiny_bvh.h:2332-2461) built over sah_split.h: the sequential host twin
// (sahbuild_host.cpp) and the level-synchronous device builder (kernels_sahbuild.hip).  Both write Wald nodes (host_builder.h: Node2) in the
// reference's non-threaded numbering — node 0 the root, node 1 unused and zero, child pairs in the pre-order of the interior nodes — and a
// primIdx in which every leaf's primitives are in ascending order.  maxLeafTris > 0: BVH::SplitLeafs( maxLeafTris ) afterwards, the new pairs
// behind the built ones in the order of the leaves they split (the reference numbers them in its own walk's order), every new node with the
// bounds of its own primitives (the reference copies the leaf's box to both halves).
// Not reproduced: the reference's printf for a large node it could not split, and its 256-entry task stack (a chain of more than 256 pending
// right children makes the reference stop splitting; neither builder here has such a limit).
#pragma once
#include <cstdint>
#include <vector>

#include "host_builder.h"

namespace tbvh {

// the number of nodes, 0 when the mesh is empty
uint32_t sah_build_host(const HostMesh& mesh, uint32_t nTris, uint32_t maxLeafTris, std::vector<Node2>& nodes, std::vector<uint32_t>& primIdx);

}  // namespace tbvh

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "mesh_source.h"

namespace tbvh {

// the small-subtree threshold of a new context (profiles/sah_device_build.txt has the sweep it was chosen from)
constexpr uint32_t kSahSmallSubtreeDefault = 64;

// device memory of one build, carved out of one allocation of sah_scratch_bytes( n ) bytes; the bins of the widest level are a second, transient
// allocation of run_sah_build's own (672 bytes per node of that level: kernels_sahbuild.hip)
size_t sah_scratch_bytes(uint32_t n, size_t* sortTempBytes, size_t* scanTempBytes);
// Builds into nodes32 (2 n nodes of two float4) and primIdx (n) on stream s; synchronises once per level (one 64-byte read-back of the counters).  *nNodesOut:
// the nodes written.  A bad vertex index of a device-resident index buffer raises kStatusMeshIndex in *status and is never dereferenced.
// smallSubtree: subtrees of at most this many primitives are finished by one wave each instead of by the per-level kernels (0: none are; a value
// of n or more: one wave builds the whole tree).  The tree does not depend on it.
hipError_t run_sah_build(const MeshSrc& verts, uint32_t n, uint32_t maxLeafTris, uint32_t smallSubtree, float4* nodes32, uint32_t* primIdx, void* scratch,
                         size_t sortTempBytes, size_t scanTempBytes, uint32_t* status, hipStream_t s, uint32_t* nNodesOut);

}  // namespace tbvh
#endif
