// kernels_mesh.hip — the two kernels that only move triangles: the BVH_GPU upload gather and tbvh_flatten_mesh_device.  Both read the
// vertices through mesh_source.h, like every other kernel that does (kernels_refit / _build / _convert / _sphere.hip).
#include "device_common.h"
#include "mesh_source.h"
#include "kernels.h"

namespace tbvh {

namespace {

// ---------------------------------------------------------------------------------------
// upload helper: gather {v0|prim, e1, e2} per primIdx entry for the BVH_GPU layout.
// e1 = v1 - v0, e2 = v2 - v0 are the same single IEEE subtractions IntersectTri performs
// per test (tiny_bvh.h:8510-8511), so pre-computing them changes no result bit.
// ---------------------------------------------------------------------------------------
template <bool GENERAL>
__global__ void k_gather_tris(const uint32_t* __restrict__ primIdx, const MeshSrc m, float4* __restrict__ out, uint64_t nIdx, uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nIdx) return;
    const uint32_t p = primIdx[i];
    float4 a, b, c;
    bool ok = p < m.nTris;   // false: slack entries of SBVH primIdx arrays (idxCount = 1.5 * triCount)
    if (ok && !mesh_tri<GENERAL>(m, p, a, b, c)) { atomicOr(status, kStatusMeshIndex); ok = false; }
    if (!ok) {
        out[i * 3] = make_float4(0, 0, 0, 0); out[i * 3 + 1] = make_float4(0, 0, 0, 0); out[i * 3 + 2] = make_float4(0, 0, 0, 0);
        return;
    }
    out[i * 3] = make_float4(a.x, a.y, a.z, as_f32(p));
    out[i * 3 + 1] = make_float4(b.x - a.x, b.y - a.y, b.z - a.z, 0.f);
    out[i * 3 + 2] = make_float4(c.x - a.x, c.y - a.y, c.z - a.z, 0.f);
}

// 3 float4 per triangle, in triangle order: what the flat-only entry points take (w: the vertex's at a 16-byte stride, else 0)
template <bool GENERAL>
__global__ void k_flatten_mesh(const MeshSrc m, float4* __restrict__ out, uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m.nTris) return;
    float4 a, b, c;
    if (!mesh_tri<GENERAL>(m, (uint32_t)i, a, b, c)) { atomicOr(status, kStatusMeshIndex); a = b = c = make_float4(0, 0, 0, 0); }
    out[i * 3] = a; out[i * 3 + 1] = b; out[i * 3 + 2] = c;
}

}  // namespace

void launch_gather_tris(const uint32_t* primIdx, const MeshSrc& m, float4* out, uint64_t nIdx, uint32_t* status, hipStream_t s) {
    const uint32_t bs = 256;
    const dim3 grid((uint32_t)((nIdx + bs - 1) / bs));
    if (m.general()) hipLaunchKernelGGL(k_gather_tris<true>, grid, dim3(bs), 0, s, primIdx, m, out, nIdx, status);
    else hipLaunchKernelGGL(k_gather_tris<false>, grid, dim3(bs), 0, s, primIdx, m, out, nIdx, status);
}

void launch_flatten_mesh(const MeshSrc& m, float4* out, uint32_t* status, hipStream_t s) {
    const uint32_t bs = 256;
    const dim3 grid((uint32_t)((m.nTris + bs - 1) / bs));
    if (m.general()) hipLaunchKernelGGL(k_flatten_mesh<true>, grid, dim3(bs), 0, s, m, out, status);
    else hipLaunchKernelGGL(k_flatten_mesh<false>, grid, dim3(bs), 0, s, m, out, status);
}

}  // namespace tbvh
