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

// The reference's three builds over BOXES fill fragment[] and call the same Build() (DESIGN.md par. 20): only where fragment i comes from differs.
//   box pairs   min = the three floats at data + i * stride + offMin, max = those at + offMax (floats): BVH::BuildAABB's bvhvec4 pairs are
//               {8, 0, 4}, the aabbMin / aabbMax of the 192-byte BLASInstance records of BVH::Build( BLASInstance*, .. ) {48, 32, 36}
//   spheres     {x, y, z, r} records, the box of the demos' sphereAABB (sah_split.h: sphere_box): BVH::Build( customGetAABB, n ) with that callback
struct SahBoxes {
    const float* data = nullptr;
    uint32_t stride = 8, offMin = 0, offMax = 4;
    bool spheres = false;
};
inline SahBoxes sah_boxes_aabbs(const void* aabbs32) { SahBoxes b; b.data = (const float*)aabbs32; return b; }
inline SahBoxes sah_boxes_instances(const void* inst192) { SahBoxes b; b.data = (const float*)inst192; b.stride = 48; b.offMin = 32; b.offMax = 36; return b; }
inline SahBoxes sah_boxes_spheres(const void* spheres16) { SahBoxes b; b.data = (const float*)spheres16; b.stride = 4; b.spheres = true; return b; }
uint32_t sah_build_host(const SahBoxes& boxes, uint32_t n, uint32_t maxLeaf, std::vector<Node2>& nodes, std::vector<uint32_t>& primIdx);

}  // namespace tbvh

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "mesh_source.h"

namespace tbvh {

// the small-subtree threshold of a new context (profiles/sah_device_build.txt has the sweep it was chosen from)
constexpr uint32_t kSahSmallSubtreeDefault = 64;
// inputs of at most this many primitives are built by one workgroup in one launch (k_sah_one_group); 0: none are.  The largest size of the sweep in
// profiles/box_sah_build.txt at which that path beat the per-level one on boxes and on triangles (at 8192 it loses on both)
constexpr uint32_t kSahOneGroupDefault = 3000;
constexpr uint32_t kSahOneGroupMax = 1u << 14;   // larger inputs take the level path whatever the threshold says: one CU is no match for them (it loses from 8192 on), and
                                                 // the scratch of an input this path may build carries its global bins, n x 672 bytes

// what the fragment step reads: triangles, or boxes in device memory
struct SahSrc {
    MeshSrc mesh;
    SahBoxes boxes;   // boxes.data != nullptr: a box source; the mesh is not read
    SahSrc(const MeshSrc& m) : mesh(m) {}
    SahSrc(const SahBoxes& b) : boxes(b) {}
};

// device memory of one build, carved out of one allocation of sah_scratch_bytes( n ) bytes; the bins of the widest level are a second, transient
// allocation of run_sah_build's own (672 bytes per node of that level: kernels_sahbuild.hip)
size_t sah_scratch_bytes(uint32_t n, size_t* sortTempBytes, size_t* scanTempBytes);
size_t sah_scratch_total(uint32_t n, size_t sortTempBytes, size_t scanTempBytes);   // the same without asking hipcub: no device needed
// Builds into nodes32 (2 n nodes of two float4) and primIdx (n) on stream s; synchronises once per level (one 64-byte read-back of the counters).  *nNodesOut:
// the nodes written.  A bad vertex index of a device-resident index buffer raises kStatusMeshIndex in *status and is never dereferenced.
// smallSubtree: subtrees of at most this many primitives are finished by one wave each instead of by the per-level kernels (0: none are; a value
// of n or more: one wave builds the whole tree).  The tree does not depend on it.
// oneGroup: n <= oneGroup builds the whole tree with one workgroup in one launch (no read-back per level; one 4-byte read-back of the node count
// at the end) instead; the tree does not depend on it either.  A broken invariant met there ends the kernel and comes back as hipErrorUnknown.
hipError_t run_sah_build(const SahSrc& src, uint32_t n, uint32_t maxLeafTris, uint32_t smallSubtree, uint32_t oneGroup, float4* nodes32, uint32_t* primIdx,
                         void* scratch, size_t sortTempBytes, size_t scanTempBytes, uint32_t* status, hipStream_t s, uint32_t* nNodesOut);

// BVH_GPU::ConvertFrom on the device (DESIGN.md par. 20): the builder's Wald nodes (nNodes of them over n primitives, max_leaf = 0 or not) as nNodes - 1
// Aila-Laine nodes of four float4 in depth-first pre-order, byte for byte what host_builder.cpp: encode_bvh_gpu gives.  scratch: the allocation the
// build ran in (its key and index arrays are free by then); asynchronous on s.
hipError_t run_al_encode(const float4* nodes32, uint32_t nNodes, uint32_t n, void* scratch, size_t sortTempBytes, size_t scanTempBytes, float4* nodes64, hipStream_t s);

}  // namespace tbvh
#endif
