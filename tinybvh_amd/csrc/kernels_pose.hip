// kernels_pose.hip — Mesh::SetPose on the device (tbvh_pose_set_skin / tbvh_pose_set_morph): one vertex per lane, the arithmetic of pose.h.
//   k_pose_skin   per vertex 48 bytes in (rest, joints, weights: three 16-byte loads, consecutive lanes consecutive addresses), 16 float4 gathered
//                 from the joint table (4 joints x 4 rows; the table is n_joints * 64 bytes, a few KB: it stays in L1 / L2 after the first wave has
//                 touched it), 16 bytes out.  A joint index >= nJoints is never used as an address: the vertex is left unwritten and reported.
//   k_pose_morph  per vertex 12 bytes per pose in (base + targets, the target loop inside the lane), 16 bytes out.  Nothing is read past vertex
//                 nVerts - 1: positions are loaded as three floats, never as a float4.
//   k_pose_skin_n / k_pose_morph_n  the same vertices (the same functions of pose.h, so the same bits) plus one posed normal per vertex into a second
//                 float4 array, for a pose with FatTri records attached: the skin normal from the blended cells the vertex uses (blended once),
//                 the morph normal the unweighted sum of the base and target normals, normalised.
//   k_pose_fat_tris  one triangle per lane: the six quarters of its FatTri that hold vN0..2 (+ Nx Ny Nz in their w) and vertex0..2 are read,
//                 rewritten from the posed corners (through the index buffer when there is one; an index >= nVerts is never used as an address: the
//                 triangle is left as it is and kStatusMeshIndex is raised) and stored; the other six quarters are not touched.
// Exact grids: one lane per vertex / triangle, the last block guarded.
#include "device_common.h"
#include "kernels.h"
#include "mesh_source.h"
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

__global__ __launch_bounds__(kPoseBlock) void k_pose_skin_n(const float4* __restrict__ rest16, const uint4* __restrict__ joints4, const float4* __restrict__ weights16,
                                                            const float4* __restrict__ mats, uint32_t nJoints, const float* __restrict__ normals12,
                                                            float4* __restrict__ out, float4* __restrict__ nOut, uint64_t nVerts, uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * kPoseBlock + threadIdx.x;
    if (i >= nVerts) return;
    const uint4 j = joints4[i];
    const float4 w = weights16[i];
    const float4 p = rest16[i];
    if (j.x >= nJoints || j.y >= nJoints || j.z >= nJoints || j.w >= nJoints) { atomicOr(status, kStatusPoseJoint); return; }
    const float nx = normals12[3 * i], ny = normals12[3 * i + 1], nz = normals12[3 * i + 2];
    const float4* m0 = mats + 4 * (uint64_t)j.x;
    const float4* m1 = mats + 4 * (uint64_t)j.y;
    const float4* m2 = mats + 4 * (uint64_t)j.z;
    const float4* m3 = mats + 4 * (uint64_t)j.w;
    float r[4], n[4];
#pragma unroll
    for (int k = 0; k < 4; k++) r[k] = pose_skin_row_n(m0[k], m1[k], m2[k], m3[k], w.x, w.y, w.z, w.w, p.x, p.y, p.z, nx, ny, nz, n[k]);
    float o[4];
    pose_skin_finish(r[0], r[1], r[2], r[3], o);
    out[i] = make_float4(o[0], o[1], o[2], o[3]);
    pose_normalize(n);
    nOut[i] = make_float4(n[0], n[1], n[2], 0.f);
}

__global__ __launch_bounds__(kPoseBlock) void k_pose_morph_n(const float* __restrict__ positions12, const float* __restrict__ weights, uint32_t nTargets,
                                                             const float* __restrict__ normals12, float4* __restrict__ out, float4* __restrict__ nOut, uint64_t nVerts) {
    const uint64_t i = (uint64_t)blockIdx.x * kPoseBlock + threadIdx.x;
    if (i >= nVerts) return;
    float o[4], n[4];
    pose_morph_vertex(positions12, nVerts, nTargets, weights, i, o);
    out[i] = make_float4(o[0], o[1], o[2], o[3]);
    pose_morph_normal(normals12, nVerts, nTargets, i, n);
    nOut[i] = make_float4(n[0], n[1], n[2], 0.f);
}

__global__ __launch_bounds__(kPoseBlock) void k_pose_fat_tris(float4* __restrict__ tris, uint64_t nTris, const float4* __restrict__ verts, const float4* __restrict__ normals,
                                                              uint64_t nVerts, const uint32_t* __restrict__ indices, int skin, uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * kPoseBlock + threadIdx.x;
    if (i >= nTris) return;
    uint64_t c[3] = {3 * i, 3 * i + 1, 3 * i + 2};
    if (indices) { c[0] = indices[3 * i]; c[1] = indices[3 * i + 1]; c[2] = indices[3 * i + 2]; }
    if (c[0] >= nVerts || c[1] >= nVerts || c[2] >= nVerts) { atomicOr(status, kStatusMeshIndex); return; }
    float4* q = tris + 12 * i;
    float t[48];                                   // (only floats 8 .. 31 are loaded, changed and stored: quarters 2 .. 7)
    float v[3][4], n[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float4 a = verts[c[k]], b = normals[c[k]];
        v[k][0] = a.x; v[k][1] = a.y; v[k][2] = a.z; n[k][0] = b.x; n[k][1] = b.y; n[k][2] = b.z;
    }
#pragma unroll
    for (int k = 2; k < 8; k++) { const float4 a = q[k]; t[4 * k] = a.x; t[4 * k + 1] = a.y; t[4 * k + 2] = a.z; t[4 * k + 3] = a.w; }
    pose_fat_tri(t, v[0], v[1], v[2], n[0], n[1], n[2], skin != 0);
#pragma unroll
    for (int k = 2; k < 8; k++) q[k] = make_float4(t[4 * k], t[4 * k + 1], t[4 * k + 2], t[4 * k + 3]);
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

void launch_pose_skin_normals(const float4* rest16, const uint4* joints4, const float4* weights16, const float4* mats, uint32_t nJoints, const float* normals12, float4* out,
                              float4* nOut, uint64_t nVerts, uint32_t* status, hipStream_t s) {
    const dim3 grid((uint32_t)((nVerts + kPoseBlock - 1) / kPoseBlock));
    hipLaunchKernelGGL(k_pose_skin_n, grid, dim3(kPoseBlock), 0, s, rest16, joints4, weights16, mats, nJoints, normals12, out, nOut, nVerts, status);
}

void launch_pose_morph_normals(const float* positions12, const float* weights, uint32_t nTargets, const float* normals12, float4* out, float4* nOut, uint64_t nVerts,
                               hipStream_t s) {
    const dim3 grid((uint32_t)((nVerts + kPoseBlock - 1) / kPoseBlock));
    hipLaunchKernelGGL(k_pose_morph_n, grid, dim3(kPoseBlock), 0, s, positions12, weights, nTargets, normals12, out, nOut, nVerts);
}

void launch_pose_fat_tris(float4* tris, uint64_t nTris, const float4* verts, const float4* normals, uint64_t nVerts, const uint32_t* indices, bool skin, uint32_t* status,
                          hipStream_t s) {
    const dim3 grid((uint32_t)((nTris + kPoseBlock - 1) / kPoseBlock));
    hipLaunchKernelGGL(k_pose_fat_tris, grid, dim3(kPoseBlock), 0, s, tris, nTris, verts, normals, nVerts, indices, skin ? 1 : 0, status);
}

}  // namespace tbvh
