// kernels_pose.hip — Mesh::SetPose on the device (tbvh_pose_set_skin / tbvh_pose_set_morph): one vertex per lane, the arithmetic of pose.h.
//   k_pose_skin   per vertex 48 bytes in (rest, joints, weights: three 16-byte loads, consecutive lanes consecutive addresses), 16 float4 gathered
//                 from the joint table (4 joints x 4 rows; the table is n_joints * 64 bytes, a few KB: it stays in L1 / L2 after the first wave has
//                 touched it), 16 bytes out.  A joint index >= nJoints is never used as an address: the vertex is left unwritten and reported.
//   k_pose_morph  per vertex 12 bytes per pose in (base + targets, the target loop inside the lane), 16 bytes out.  Nothing is read past vertex
//                 nVerts - 1: positions are loaded as three floats, never as a float4.
// Exact grids: one lane per vertex, the last block guarded.
#include "device_common.h"
#include "kernels.h"
#include "pose.h"

namespace tbvh {

namespace {

constexpr uint32_t kPoseBlock = 256;

__global__ __launch_bounds__(kPoseBlock) void k_pose_skin(const float4* __restrict__ rest16, const uint4* __restrict__ joints4, const float4* __restrict__ weights16,
                                                          const float4* __restrict__ mats, uint32_t nJoints, float4* __restrict__ out, uint64_t nVerts,
                                                          uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * kPoseBlock + threadIdx.x;
    if (i >= nVerts) return;
    const uint4 j = joints4[i];
    const float4 w = weights16[i];
    const float4 p = rest16[i];
    if (j.x >= nJoints || j.y >= nJoints || j.z >= nJoints || j.w >= nJoints) { atomicOr(status, kStatusPoseJoint); return; }
    const float4* m0 = mats + 4 * (uint64_t)j.x;
    const float4* m1 = mats + 4 * (uint64_t)j.y;
    const float4* m2 = mats + 4 * (uint64_t)j.z;
    const float4* m3 = mats + 4 * (uint64_t)j.w;
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; k++) r[k] = pose_skin_row(m0[k], m1[k], m2[k], m3[k], w.x, w.y, w.z, w.w, p.x, p.y, p.z);
    float o[4];
    pose_skin_finish(r[0], r[1], r[2], r[3], o);
    out[i] = make_float4(o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(kPoseBlock) void k_pose_morph(const float* __restrict__ positions12, const float* __restrict__ weights, uint32_t nTargets,
                                                           float4* __restrict__ out, uint64_t nVerts) {
    const uint64_t i = (uint64_t)blockIdx.x * kPoseBlock + threadIdx.x;
    if (i >= nVerts) return;
    float o[4];
    pose_morph_vertex(positions12, nVerts, nTargets, weights, i, o);
    out[i] = make_float4(o[0], o[1], o[2], o[3]);
}

}  // namespace

void launch_pose_skin(const float4* rest16, const uint4* joints4, const float4* weights16, const float4* mats, uint32_t nJoints, float4* out, uint64_t nVerts,
                      uint32_t* status, hipStream_t s) {
    const dim3 grid((uint32_t)((nVerts + kPoseBlock - 1) / kPoseBlock));
    hipLaunchKernelGGL(k_pose_skin, grid, dim3(kPoseBlock), 0, s, rest16, joints4, weights16, mats, nJoints, out, nVerts, status);
}

void launch_pose_morph(const float* positions12, const float* weights, uint32_t nTargets, float4* out, uint64_t nVerts, hipStream_t s) {
    const dim3 grid((uint32_t)((nVerts + kPoseBlock - 1) / kPoseBlock));
    hipLaunchKernelGGL(k_pose_morph, grid, dim3(kPoseBlock), 0, s, positions12, weights, nTargets, out, nVerts);
}

}  // namespace tbvh
