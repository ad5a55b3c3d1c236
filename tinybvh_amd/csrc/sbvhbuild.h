// sbvhbuild.h — the reference's spatial-split tree (SBVH: BVH::BuildHQ, tiny_bvh.h:2623-3040) built over sbvh_split.h: the sequential host twin
// (sbvhbuild_host.cpp) and the level-synchronous device builder (kernels_sbvhbuild.hip).  DESIGN.md §19.
//
// Both write what BuildHQ leaves after its final Compact(): Wald nodes (host_builder.h: Node2) — node 0 the root, node 1 unused and zero, child
// pairs in the pre-order of the interior nodes — and primIdx = the references the leaves hold, consecutive from 0 in that walk's leaf order, each
// leaf in the order the reference's partition left it (a triangle that was split is named by several leaves).  At most n + n / 2 references and
// 3 n nodes.  With maxLeafTris = 0 these are the reference's bytes (threaded or not: Compact makes the numbering canonical).
// maxLeafTris > 0: afterwards every leaf of more than that many references becomes a chain of pairs behind the built nodes, as sahbuild.h does it,
// each new node with the bounds of its triangles INTERSECTED with the leaf's box (a clipped leaf must not grow back).
//
// One path of the reference is NOT reproduced: when a partition leaves one side empty ("spatial split failed. We shouldn't get here", 2967-2975: a
// spatial split that failed, or an object split of coordinates whose areas overflow) the reference reads primIdx entries that may be stale scratch.  Both builders here make that node a leaf over its fragments in
// partition order with the refreshed bounds and count it in Stats::failedPartitions; byte equality with the reference is not promised for a tree
// where that count is not zero (it is zero on every scene the tests compare with the reference).
// Also not reproduced: the 512-entry localTask stack and Compact's 128-entry stack (neither builder here has a depth limit), hqbvhoddeven and bin
// counts other than 8.
#pragma once
#include <cstdint>
#include <vector>

#include "host_builder.h"
#include "sbvh_split.h"

namespace tbvh {

// the number of nodes, 0 when the mesh is empty.  stats may be null.
uint32_t sbvh_build_host(const HostMesh& mesh, uint32_t nTris, uint32_t maxLeafTris, std::vector<Node2>& nodes, std::vector<uint32_t>& primIdx,
                         sbvh::Stats* stats);

}  // namespace tbvh

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "mesh_source.h"

namespace tbvh {

// device memory of one build, carved out of one allocation of sbvh_scratch_bytes( n ) bytes
size_t sbvh_scratch_bytes(uint32_t n, size_t* scanTempBytes);
size_t sbvh_scratch_total(uint32_t n, size_t scanTempBytes);   // the same without asking hipcub: no device needed
// Builds into nodes32 (room for 3 n nodes of two float4) and primIdx (room for n + n / 2) on stream s; synchronises once per level (one small
// read-back of the counters).  *nNodesOut, *nIdxOut: the nodes and references written; *stats (may be null): what the twin counts.  A bad vertex
// index of a device-resident index buffer raises kStatusMeshIndex in *status and is never dereferenced.
hipError_t run_sbvh_build(const MeshSrc& verts, uint32_t n, uint32_t maxLeafTris, float4* nodes32, uint32_t* primIdx, void* scratch, size_t scanTempBytes,
                          uint32_t* status, hipStream_t s, uint32_t* nNodesOut, uint32_t* nIdxOut, sbvh::Stats* stats);

}  // namespace tbvh
#endif
