// capi_mesh.hip — indexed and strided triangle meshes (tbvh_mesh): validation, the device view every kernel launch takes (mesh_source.h), and the
// entry points that are nothing but their flat counterpart with the mesh carried through (host build / upload, sphere queries, flatten).  The scene
// side — upload, update, device build / conversion, refit — is in capi_scene.hip next to the flat calls, which run the same code with a flat source.
#include "capi_internal.h"

using namespace tbvh;
using namespace tbvh_capi;

namespace tbvh_capi {

tbvh_mesh flatMesh(const void* verts16, uint64_t nTris, int onDevice) {
    tbvh_mesh m;
    m.verts = verts16; m.n_verts = nTris * 3; m.stride_bytes = 16; m.on_device = onDevice ? 1u : 0u; m.indices = nullptr; m.n_tris = nTris;
    return m;
}

uint64_t meshVertexBytes(const tbvh_mesh& m) {
    const uint32_t stride = m.stride_bytes ? m.stride_bytes : 16u;
    return m.n_verts ? (m.n_verts - 1) * stride + (stride == 16u ? 16u : 12u) : 0;
}

int checkMesh(const tbvh_mesh* m, const char* who, bool indicesMayBeHeld) {
    if (!m || !m->verts || m->n_tris == 0 || m->n_verts == 0) return fail(TBVH_E_INVALID, "%s: null/empty mesh", who);
    const uint32_t stride = m->stride_bytes ? m->stride_bytes : 16u;
    if (stride % 4u || stride < 12u) return fail(TBVH_E_INVALID, "%s: stride_bytes %u (0 = 16, or a multiple of 4 that is >= 12)", who, m->stride_bytes);
    if (m->n_verts >> 32 || (m->n_tris * 3) >> 32 || m->n_tris >> 32)
        return fail(TBVH_E_INVALID, "%s: %llu vertices, %llu triangles: vertex indices are 32-bit", who, (unsigned long long)m->n_verts, (unsigned long long)m->n_tris);
    if (!m->indices && !indicesMayBeHeld && m->n_verts < m->n_tris * 3)
        return fail(TBVH_E_INVALID, "%s: %llu triangles without indices need %llu vertices, the mesh has %llu", who, (unsigned long long)m->n_tris,
                    (unsigned long long)(m->n_tris * 3), (unsigned long long)m->n_verts);
    if (m->on_device) {
        if ((uintptr_t)m->verts & (stride == 16u ? 15u : 3u)) return fail(TBVH_E_INVALID, "%s: device vertices must be %u-byte aligned at this stride", who, stride == 16u ? 16u : 4u);
        if ((uintptr_t)m->indices & 3u) return fail(TBVH_E_INVALID, "%s: device indices must be 4-byte aligned", who);
        return 0;   // (device-resident indices are checked by the kernels that read them)
    }
    if (m->indices)
        for (uint64_t i = 0; i < m->n_tris * 3; i++)
            if (m->indices[i] >= m->n_verts)
                return fail(TBVH_E_FORMAT, "%s: triangle %llu: vertex index %u is not a vertex (%llu vertices)", who, (unsigned long long)(i / 3), m->indices[i], (unsigned long long)m->n_verts);
    return 0;
}

int stageMesh(tbvh_context* c, const tbvh_mesh& m, DeviceMesh& out) {
    out.src.nTris = m.n_tris; out.src.nVerts = (uint32_t)m.n_verts; out.src.stride = m.stride_bytes ? m.stride_bytes : 16u;
    if (m.on_device) { out.src.verts = (const float4*)m.verts; out.src.indices = m.indices; return 0; }
    const uint64_t vb = meshVertexBytes(m);
    HIP_TRY(out.ownVerts.alloc(vb ? vb : 16));
    if (vb) HIP_TRY(hipMemcpyAsync(out.ownVerts, m.verts, vb, hipMemcpyHostToDevice, c->stream));
    out.src.verts = (const float4*)out.ownVerts.get();
    if (m.indices) {
        HIP_TRY(out.ownIdx.alloc(m.n_tris * 3));
        HIP_TRY(hipMemcpyAsync(out.ownIdx, m.indices, m.n_tris * 12, hipMemcpyHostToDevice, c->stream));
        out.src.indices = out.ownIdx;
    }
    return 0;
}

int keepMeshIndices(tbvh_scene* s, const MeshSrc& src) {
    if (!src.indices) return 0;
    if (s->meshIdx && s->meshIdxTris != src.nTris) {
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        s->meshIdx.reset(); s->meshIdxTris = 0;
    }
    if (!s->meshIdx) {
        HIP_TRY(s->meshIdx.alloc(src.nTris * 3));
        s->meshIdxTris = src.nTris;
    }
    HIP_TRY(hipMemcpyAsync(s->meshIdx, src.indices, src.nTris * 12, hipMemcpyDeviceToDevice, s->ctx->stream));
    return 0;
}

}  // namespace tbvh_capi

extern "C" {

// ---- host builder ---------------------------------------------------------------------------------------------------------------------

int tbvh_host_build_mesh(const tbvh_mesh* mesh, int layout, const tbvh_build_params* p, tbvh_hostbvh** out) {
    if (!out) return fail(TBVH_E_INVALID, "tbvh_host_build_mesh: null argument");
    if (mesh && mesh->on_device) return fail(TBVH_E_INVALID, "tbvh_host_build_mesh: the host builder reads host memory (on_device = 0)");
    if (int r = checkMesh(mesh, "tbvh_host_build_mesh")) return r;
    return hostBuildImpl(HostMesh(mesh->verts, mesh->stride_bytes, mesh->indices), mesh->n_tris, layout, p, out);
}

int tbvh_upload_host_mesh(tbvh_context* c, const tbvh_hostbvh* h, const tbvh_mesh* mesh, tbvh_scene** out) {
    if (!c || !h || !out) return fail(TBVH_E_INVALID, "tbvh_upload_host_mesh: null argument");
    if (int r = checkMesh(mesh, "tbvh_upload_host_mesh")) return r;
    if (h->bvh2.triCount && h->bvh2.triCount != mesh->n_tris)   // (a blob read from a file has no BVH2 and no count to compare)
        return fail(TBVH_E_INVALID, "tbvh_upload_host_mesh: the mesh has %llu triangles, the host BVH was built over %u", (unsigned long long)mesh->n_tris, h->bvh2.triCount);
    if (h->layout == TBVH_LAYOUT_BVH_GPU)
        return tbvh_upload_bvh_gpu_mesh(c, h->al.data(), h->al.size(), h->bvh2.primIdx.data(), h->bvh2.primIdx.size(), mesh, out);
    if (h->layout != TBVH_LAYOUT_BVH4_GPU && h->layout != TBVH_LAYOUT_CWBVH) return fail(TBVH_E_INVALID, "layout %d cannot be uploaded", h->layout);
    // the wide blobs carry their triangles: nothing of the mesh is read, but an indexed mesh leaves the scene its index buffer (tbvh_refit_mesh)
    tbvh_scene* s = nullptr;
    if (int r = tbvh_upload_host(c, h, nullptr, 0, &s)) return r;
    if (mesh->indices) {
        TBVH_ENTER(c);
        MeshSrc only;
        DevBuf<uint32_t> tmp;
        only.nTris = mesh->n_tris; only.indices = mesh->indices;
        int r = 0;
        if (!mesh->on_device) {
            if (tmp.alloc(mesh->n_tris * 3) != hipSuccess || hipMemcpyAsync(tmp, mesh->indices, mesh->n_tris * 12, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
                (void)hipGetLastError(); r = fail(TBVH_E_NOMEM, "tbvh_upload_host_mesh: %llu bytes of device memory for the index buffer", (unsigned long long)(mesh->n_tris * 12));
            }
            only.indices = tmp;
        }
        if (!r) r = keepMeshIndices(s, only);
        hipStreamSynchronize(c->stream);   // (the copy out of the temporary is done before it goes)
        if (r) { tbvh_free_scene(s); return r; }
    }
    *out = s;
    return 0;
}

// ---- sphere queries -------------------------------------------------------------------------------------------------------------------

int tbvh_intersect_spheres_mesh_device(tbvh_scene* s, const void* dSpheres, uint64_t n, const tbvh_mesh* mesh, uint8_t* dHit) {
    if (int r = checkSphereScene(s, "tbvh_intersect_spheres_mesh_device")) return r;
    if (n == 0) return 0;
    if (!dSpheres || !dHit) return fail(TBVH_E_INVALID, "tbvh_intersect_spheres_mesh_device: null argument");
    if (int r = checkMesh(mesh, "tbvh_intersect_spheres_mesh_device")) return r;
    if (!mesh->on_device) return fail(TBVH_E_INVALID, "tbvh_intersect_spheres_mesh_device: the mesh must be device memory (on_device = 1)");
    if ((uintptr_t)dSpheres & 15) return fail(TBVH_E_INVALID, "tbvh_intersect_spheres_mesh_device: the sphere array must be 16-byte aligned");
    TBVH_ENTER(s->ctx);
    DeviceMesh dm;
    if (int r = stageMesh(s->ctx, *mesh, dm)) return r;   // (device-resident: used in place, nothing is copied)
    return launchSpheres(s, (const float4*)dSpheres, n, dm.src, dHit);
}

int tbvh_intersect_spheres_mesh(tbvh_scene* s, const void* spheres, uint64_t n, const tbvh_mesh* mesh, uint8_t* hit) {
    if (int r = checkSphereScene(s, "tbvh_intersect_spheres_mesh")) return r;
    if (n == 0) return 0;
    if (!spheres || !hit) return fail(TBVH_E_INVALID, "tbvh_intersect_spheres_mesh: null argument");
    if (int r = checkMesh(mesh, "tbvh_intersect_spheres_mesh")) return r;
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    if (int r = ensureStage(c, (n + 3) / 4)) return r;
    if (int r = ensureStageOcc(c, n)) return r;
    // a host mesh goes up through the scene's staging buffers (the vertex one is tbvh_refit's and tbvh_intersect_spheres'), grown when needed and kept
    MeshSrc src;
    src.nTris = mesh->n_tris; src.nVerts = (uint32_t)mesh->n_verts; src.stride = mesh->stride_bytes ? mesh->stride_bytes : 16u;
    src.verts = (const float4*)mesh->verts; src.indices = mesh->indices;
    if (!mesh->on_device) {
        const uint64_t vb = meshVertexBytes(*mesh), ib = mesh->indices ? mesh->n_tris * 12 : 0;
        HIP_TRY(s->vertStage.reserve(vb));
        HIP_TRY(s->idxStage.reserve(ib / 4));
        HIP_TRY(hipMemcpyAsync(s->vertStage, mesh->verts, vb, hipMemcpyHostToDevice, c->stream));
        if (ib) HIP_TRY(hipMemcpyAsync(s->idxStage, mesh->indices, ib, hipMemcpyHostToDevice, c->stream));
        src.verts = (const float4*)s->vertStage.get(); src.indices = ib ? s->idxStage.get() : nullptr;
    }
    HIP_TRY(hipMemcpyAsync(c->stageRays, spheres, n * 16, hipMemcpyHostToDevice, c->stream));
    int r = launchSpheres(s, (const float4*)c->stageRays.get(), n, src, c->stageOcc);
    if (!r && hipMemcpyAsync(hit, c->stageOcc, n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) r = fail(TBVH_E_HIP, "tbvh_intersect_spheres_mesh: copy from the device failed");
    if (!r) return checkStatus(c);   // (synchronizes)
    hipStreamSynchronize(c->stream);
    return r;
}

// ---- flatten --------------------------------------------------------------------------------------------------------------------------

int tbvh_flatten_mesh_device(tbvh_context* c, const tbvh_mesh* mesh, void* dOut) {
    if (!c || !dOut) return fail(TBVH_E_INVALID, "tbvh_flatten_mesh_device: null argument");
    if ((uintptr_t)dOut & 15) return fail(TBVH_E_INVALID, "tbvh_flatten_mesh_device: the output must be 16-byte aligned");
    if (int r = checkMesh(mesh, "tbvh_flatten_mesh_device")) return r;
    TBVH_ENTER(c);
    DeviceMesh dm;
    if (int r = stageMesh(c, *mesh, dm)) return r;
    launch_flatten_mesh(dm.src, (float4*)dOut, c->status, c->stream);
    HIP_TRY(hipGetLastError());
    if (!mesh->on_device) return checkStatus(c);   // (the staged copy goes with this call)
    return 0;
}

}  // extern "C"
