// kernels_scenegraph.hip — Scene::UpdateSceneGraph on the device (tbvh_scenegraph_*): the work items of scenegraph.h, one per lane.  The problem is small
// and latency-bound (a drone: 100 channels, 93 nodes), so the aim is few launches and no host round trip, not occupancy: one advance is four launches.
//   k_graph_sample   one channel per lane: reads and writes its (t, k), walks k forward as Channel::Update does, samples, and — unless a later channel
//                    writes the same field — stores the node's T, R or S (or its weights) and the node's "written" mark.
//   k_graph_local    one node per lane: T * R * S * matrix for the nodes marked since the last walk; the mark is cleared.
//   k_graph_combine  one node per lane: identity * local[root] * ... * local[node], multiplied down the node's own ancestor chain.  These are the products
//                    Node::Update's recursion performs for that node, left to right, so the bits are the same; ancestors shared by many lanes are multiplied
//                    again by each, which buys one launch for the whole tree and no dependency between lanes.  A launch per depth level over depth-sorted nodes (no
//                    repeated products) was built and measured against this: 4x slower at 93 nodes / depth 20, 3.5x at 102 k nodes / depth 25
//                    (profiles/scenegraph_anim.txt), and deleted.
//   k_graph_outputs  lanes [0, nInstances): the instance's node's combined matrix, copied; lanes [nInstances, + nPairs): one (skin use, joint) pair:
//                    inverse( mesh node ) * joint node * inverseBind, the inverse recomputed per lane with the same operations.
//   k_graph_set_time Animation::SetTime / Reset over one animation's channels.
// Every index taken from an array is compared with its bound before an address is formed (scenegraph.h); a violation leaves the item unwritten and raises
// kStatusGraph.  Exact grids of 256-lane blocks, the last block guarded; no LDS.  The tables are read through the kernel argument's global pointers.
#include "device_common.h"
#include "kernels.h"
#include "scenegraph.h"

namespace tbvh {

namespace {

constexpr uint32_t kGraphBlock = 256;

__global__ __launch_bounds__(kGraphBlock) void k_graph_sample(const SgView g, uint32_t c0, uint32_t c1, float dt, uint32_t shadowMask) {
    const uint32_t c = c0 + blockIdx.x * kGraphBlock + threadIdx.x;
    if (c >= c1 || c >= g.nChannels) return;
    sg_channel(g, c, dt, shadowMask);
}

__global__ __launch_bounds__(kGraphBlock) void k_graph_local(const SgView g) {
    const uint32_t n = blockIdx.x * kGraphBlock + threadIdx.x;
    if (n >= g.nNodes) return;
    sg_node_local(g, n);
}

__global__ __launch_bounds__(kGraphBlock) void k_graph_combine(const SgView g) {
    const uint32_t n = blockIdx.x * kGraphBlock + threadIdx.x;
    if (n >= g.nNodes) return;
    sg_node_combine(g, n);
}

__global__ __launch_bounds__(kGraphBlock) void k_graph_outputs(const SgView g) {
    const uint32_t i = blockIdx.x * kGraphBlock + threadIdx.x;
    if (i < g.nInstances) sg_instance(g, i);
    else if (i - g.nInstances < g.nPairs) sg_joint_pair(g, i - g.nInstances);
}

__global__ __launch_bounds__(kGraphBlock) void k_graph_set_time(float* __restrict__ cT, int32_t* __restrict__ cK, uint32_t c0, uint32_t c1, float t) {
    const uint32_t c = c0 + blockIdx.x * kGraphBlock + threadIdx.x;
    if (c >= c1) return;
    cT[c] = t; cK[c] = 0;
}

__global__ void k_graph_set_local(float* __restrict__ local, uint32_t node, const SgMat m) {
    if (threadIdx.x < 16) local[16 * (uint64_t)node + threadIdx.x] = m.m[threadIdx.x];
}

inline dim3 gridFor(uint64_t n) { return dim3((uint32_t)((n + kGraphBlock - 1) / kGraphBlock)); }

}  // namespace

void launch_graph_sample(const SgView& g, uint32_t c0, uint32_t c1, float dt, uint32_t shadowMask, hipStream_t s) {
    if (c1 <= c0) return;
    hipLaunchKernelGGL(k_graph_sample, gridFor(c1 - c0), dim3(kGraphBlock), 0, s, g, c0, c1, dt, shadowMask);
}

void launch_graph_walk(const SgView& g, int only, hipStream_t s) {
    if (only < 0 || only == 1) hipLaunchKernelGGL(k_graph_local, gridFor(g.nNodes), dim3(kGraphBlock), 0, s, g);
    if (only < 0 || only == 2) hipLaunchKernelGGL(k_graph_combine, gridFor(g.nNodes), dim3(kGraphBlock), 0, s, g);
    const uint64_t nOut = (uint64_t)g.nInstances + g.nPairs;
    if (nOut && (only < 0 || only == 3)) hipLaunchKernelGGL(k_graph_outputs, gridFor(nOut), dim3(kGraphBlock), 0, s, g);
}

void launch_graph_set_time(float* cT, int32_t* cK, uint32_t c0, uint32_t c1, float t, hipStream_t s) {
    if (c1 <= c0) return;
    hipLaunchKernelGGL(k_graph_set_time, gridFor(c1 - c0), dim3(kGraphBlock), 0, s, cT, cK, c0, c1, t);
}

void launch_graph_set_local(float* local, uint32_t node, const SgMat& m, hipStream_t s) {
    hipLaunchKernelGGL(k_graph_set_local, dim3(1), dim3(64), 0, s, local, node, m);
}

}  // namespace tbvh
