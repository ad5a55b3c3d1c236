// mesh_source.h — where a kernel finds a triangle's three vertices: the device side of tbvh_mesh (include/tinybvh_amd.h), i.e. of the
// reference's bvhvec4slice { data, count, stride } + BVH::vertIdx (tiny_bvh.h:428-436, 1659-1661).  Every kernel that reads vertices — the
// BVH_GPU gather, the refit kernels, the device builders' triangle boxes, the leaf writers of the device conversion, the sphere-overlap
// triangle test — fetches through mesh_tri below, and is compiled twice:
//   GENERAL = false   today's form, 3 float4 per triangle at verts[3 p + k]: three independent 16-byte loads, nothing else.  The caller has
//                     checked p < nTris, as it always did.
//   GENERAL = true    an index buffer (3 per triangle) and / or a vertex stride other than 16 bytes: the three indices are loaded first (one
//                     12-byte run per lane: one global_load_dwordx3), then the three vertices — three independent chains, issued together.
//                     x, y, z are one 12-byte load per vertex; w is a fourth dword read ONLY at a 16-byte stride (the compiler merges the two
//                     arms of mesh_vertex into dwordx3 + a conditional dword at offset 12, same cache line), any other stride gives w = 0, so
//                     the last vertex of an interleaved buffer needs no 4 bytes behind it.  `wide` is uniform over the launch.
//                     An index >= nVerts is never dereferenced: the fetch fails and the kernel reports it (status |= kStatusMeshIndex).
// Which instance runs is decided on the host per launch (MeshSrc::general), so the flat path does not pay for the general one.
#pragma once
#include "device_common.h"

namespace tbvh {

constexpr uint32_t kStatusMeshIndex = 32u;   // status word: a vertex index of a device-resident index buffer is >= n_verts (capi_query.hip: checkStatus)

struct MeshSrc {
    const float4* verts = nullptr;     // flat: 3 float4 per triangle; general: the address of vertex 0
    const uint32_t* indices = nullptr; // 3 per triangle, or nullptr: triangle p = vertices 3 p, 3 p + 1, 3 p + 2
    uint64_t nTris = 0;
    uint32_t nVerts = 0;               // general form only: indices are checked against it
    uint32_t stride = 16;              // bytes between vertices
    bool general() const { return indices != nullptr || stride != 16u; }
};

inline MeshSrc flat_mesh(const float4* verts16, uint64_t nTris) {
    MeshSrc m;
    m.verts = verts16; m.nTris = nTris; m.nVerts = (uint32_t)(nTris * 3 > 0xffffffffull ? 0xffffffffull : nTris * 3);
    return m;
}

#if defined(__HIPCC__)
__device__ __forceinline__ float4 mesh_vertex(const MeshSrc& m, uint32_t j, bool wide) {
    const char* p = (const char*)m.verts + (size_t)j * m.stride;
    if (wide) return *(const float4*)p;
    const float* f = (const float*)p;
    return make_float4(f[0], f[1], f[2], 0.f);
}

// the three vertices of triangle p; false (GENERAL only): an index is out of range, nothing was read through it
template <bool GENERAL>
__device__ __forceinline__ bool mesh_tri(const MeshSrc& m, uint32_t p, float4& v0, float4& v1, float4& v2) {
    if (!GENERAL) {
        v0 = m.verts[3 * (uint64_t)p]; v1 = m.verts[3 * (uint64_t)p + 1]; v2 = m.verts[3 * (uint64_t)p + 2];
        return true;
    }
    uint64_t i0 = 3 * (uint64_t)p, i1 = i0 + 1, i2 = i0 + 2;
    if (m.indices) { const uint32_t* ip = m.indices + 3 * (uint64_t)p; i0 = ip[0]; i1 = ip[1]; i2 = ip[2]; }
    if (i0 >= m.nVerts || i1 >= m.nVerts || i2 >= m.nVerts) return false;
    const bool wide = m.stride == 16u;
    v0 = mesh_vertex(m, (uint32_t)i0, wide); v1 = mesh_vertex(m, (uint32_t)i1, wide); v2 = mesh_vertex(m, (uint32_t)i2, wide);
    return true;
}
#endif

}  // namespace tbvh
