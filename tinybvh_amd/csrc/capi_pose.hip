// capi_pose.hip — skinned and morph-target meshes posed on the device (tbvh_pose_*; include/tinybvh_amd.h, DESIGN.md par. 14): Mesh::SetPose of
// tiny_scene.h, the vertex part.  A pose owns its rest data and one output vertex buffer; per frame the joint matrices or the morph weights go up
// through a small pinned staging area (two slots, so that a frame's copy does not wait for the previous frame's), the kernel of kernels_pose.hip
// writes the vertices, and tbvh_pose_refit hands them to tbvh_refit / tbvh_refit_mesh as device-resident vertices.  The host variants (tbvh_host_pose_*: the same
// header on the CPU) are in pose_host.cpp.
#include "capi_internal.h"
#include "pose.h"

using namespace tbvh;
using namespace tbvh_capi;

struct tbvh_pose {
    tbvh_context* ctx = nullptr;
    int kind = 0;                    // 1 skin, 2 morph
    uint64_t nVerts = 0;
    uint32_t nJoints = 0, nTargets = 0;
    DevBuf<float4> rest, weights;    // skin: one per vertex
    DevBuf<uint4> joints;
    DevBuf<float> positions;         // morph: (nTargets + 1) * nVerts * 3
    DevBuf<float> params;            // skin: nJoints * 16 floats (the joint table); morph: nTargets weights
    DevBuf<float4> out;              // nVerts posed vertices
    // FatTri records attached (tbvh_pose_attach_fat_tris): every tbvh_pose_set_* also rewrites the records of `slot` of `shading` (looked up per call: the
    // slot may have been set again since).  normals: skin nVerts * 3 rest normals, morph (nTargets + 1) * nVerts * 3; nOut: one posed normal per vertex
    tbvh_shading* shading = nullptr;
    uint32_t slot = 0;
    uint64_t fatTris = 0;
    DevBuf<float> normals;
    DevBuf<float4> nOut;
    DevBuf<uint32_t> fatIdx;         // 3 per triangle, or empty: triangle i has corners 3i .. 3i + 2
    // host matrices / weights are copied here before tbvh_pose_set_* returns and go up by DMA from here; a slot is reused once its copy has left
    char* pin = nullptr;
    uint64_t pinSlotBytes = 0;
    hipEvent_t pinEv[2] = {nullptr, nullptr};
    bool pinUsed[2] = {false, false};
    int pinCur = 0;
};

namespace {

enum { kPoseSkin = 1, kPoseMorph = 2 };

int allocFail(const char* who, uint64_t bytes) {
    (void)hipGetLastError();
    return fail(TBVH_E_NOMEM, "%s: %llu bytes of device memory", who, (unsigned long long)bytes);
}

int makeStaging(tbvh_pose* p, uint64_t paramBytes) {
    p->pinSlotBytes = (paramBytes + 63) & ~63ull;
    if (!p->pinSlotBytes) return 0;   // (a morph pose without targets has nothing to send)
    if (hipHostMalloc((void**)&p->pin, 2 * p->pinSlotBytes) != hipSuccess) { (void)hipGetLastError(); p->pin = nullptr; return fail(TBVH_E_NOMEM, "tbvh_pose: %llu bytes of pinned host memory for the parameter staging area", (unsigned long long)(2 * p->pinSlotBytes)); }
    for (int k = 0; k < 2; k++) HIP_TRY(hipEventCreateWithFlags(&p->pinEv[k], hipEventDisableTiming));
    return 0;
}

// the pose's parameter array on the device: where the caller has it, or staged (the caller's array is free on return)
int stageParams(tbvh_pose* p, const float* src, uint64_t bytes, int onDevice, const float** dev) {
    if (onDevice || !bytes) { *dev = src; return 0; }
    tbvh_context* c = p->ctx;
    const int slot = p->pinCur;
    if (p->pinUsed[slot]) HIP_TRY(hipEventSynchronize(p->pinEv[slot]));
    char* h = p->pin + (uint64_t)slot * p->pinSlotBytes;
    memcpy(h, src, bytes);
    HIP_TRY(hipMemcpyAsync(p->params, h, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(p->pinEv[slot], c->stream));
    p->pinUsed[slot] = true; p->pinCur ^= 1;
    *dev = p->params;
    return 0;
}

void destroyPose(tbvh_pose* p) {
    for (hipEvent_t e : p->pinEv) if (e) hipEventDestroy(e);
    if (p->pin) hipHostFree(p->pin);
    delete p;
}

}  // namespace

namespace {
// tbvh_pose_set_* with records attached: the slot's records as they are now, refused before anything is staged or launched when their number changed
int attachedRecords(tbvh_pose* p, const char* who, float4** tris) {
    *tris = nullptr;
    if (!p->shading) return 0;
    uint64_t n = 0;
    shadingSlotRecords(p->shading, p->slot, tris, &n);
    if (n != p->fatTris) return fail(TBVH_E_INVALID, "%s: slot %u of the attached shading table now holds %llu records, the pose was attached to %llu", who, p->slot, (unsigned long long)n, (unsigned long long)p->fatTris);
    return 0;
}
// ... and its tail: the records follow the vertices and normals just posed (inside the same timed operation)
void updateFatTris(tbvh_pose* p, float4* tris) {
    launch_pose_fat_tris(tris, p->fatTris, p->out, p->nOut, p->nVerts, p->fatIdx ? p->fatIdx.get() : nullptr, p->kind == kPoseSkin, p->ctx->status, p->ctx->stream);
}
}  // namespace

namespace tbvh_capi {
void detachPosesFrom(tbvh_context* c, const tbvh_shading* sh) {
    for (tbvh_pose* p : c->poses)
        if (p->shading == sh) { p->shading = nullptr; p->normals.reset(); p->nOut.reset(); p->fatIdx.reset(); p->fatTris = 0; }
}
void freePosesOf(tbvh_context* c) {
    for (tbvh_pose* p : c->poses) destroyPose(p);
    c->poses.clear();
}
}  // namespace tbvh_capi

extern "C" {

int tbvh_pose_create_skin(tbvh_context* c, const void* rest16, uint64_t nVerts, const uint32_t* joints4, const void* weights16, uint32_t nJoints,
                          int onDevice, tbvh_pose** out) {
    if (!c || !rest16 || !joints4 || !weights16 || !out) return fail(TBVH_E_INVALID, "tbvh_pose_create_skin: null argument");
    if (nVerts == 0 || nVerts >> 32 || nJoints == 0) return fail(TBVH_E_INVALID, "tbvh_pose_create_skin: %llu vertices, %u joints", (unsigned long long)nVerts, nJoints);
    if (onDevice) {
        if (((uintptr_t)rest16 | (uintptr_t)joints4 | (uintptr_t)weights16) & 15) return fail(TBVH_E_INVALID, "tbvh_pose_create_skin: device arrays must be 16-byte aligned");
    } else {
        const uint64_t bad = pose_first_bad_joint(joints4, nVerts, nJoints);   // before anything is allocated
        if (bad != nVerts)
            return fail(TBVH_E_FORMAT, "tbvh_pose_create_skin: vertex %llu: a joint index (%u %u %u %u) is not a joint (%u joints)", (unsigned long long)bad, joints4[4 * bad],
                        joints4[4 * bad + 1], joints4[4 * bad + 2], joints4[4 * bad + 3], nJoints);
    }
    TBVH_ENTER(c);
    tbvh_pose* p = new (std::nothrow) tbvh_pose;
    if (!p) return fail(TBVH_E_NOMEM, "tbvh_pose_create_skin: out of host memory");
    p->ctx = c; p->kind = kPoseSkin; p->nVerts = nVerts; p->nJoints = nJoints;
    if (p->rest.alloc(nVerts) != hipSuccess || p->weights.alloc(nVerts) != hipSuccess || p->joints.alloc(nVerts) != hipSuccess || p->out.alloc(nVerts) != hipSuccess ||
        p->params.alloc((size_t)nJoints * 16) != hipSuccess) {
        destroyPose(p);
        return allocFail("tbvh_pose_create_skin", nVerts * 64 + (uint64_t)nJoints * 64);   // (rest, joints, weights, output; the joint table)
    }
    int r = makeStaging(p, (uint64_t)nJoints * 64);
    const hipMemcpyKind kind = onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (!r && (hipMemcpyAsync(p->rest, rest16, nVerts * 16, kind, c->stream) != hipSuccess || hipMemcpyAsync(p->joints, joints4, nVerts * 16, kind, c->stream) != hipSuccess ||
               hipMemcpyAsync(p->weights, weights16, nVerts * 16, kind, c->stream) != hipSuccess || hipMemsetAsync(p->out, 0, nVerts * 16, c->stream) != hipSuccess ||
               hipStreamSynchronize(c->stream) != hipSuccess))
        r = fail(TBVH_E_HIP, "tbvh_pose_create_skin: copying the rest data failed: %s", hipGetErrorString(hipGetLastError()));
    if (r) { destroyPose(p); return r; }
    c->poses.push_back(p);
    *out = p;
    return 0;
}

int tbvh_pose_create_morph(tbvh_context* c, const float* positions12, uint64_t nVerts, uint32_t nTargets, int onDevice, tbvh_pose** out) {
    if (!c || !positions12 || !out) return fail(TBVH_E_INVALID, "tbvh_pose_create_morph: null argument");
    if (nVerts == 0 || nVerts >> 32) return fail(TBVH_E_INVALID, "tbvh_pose_create_morph: %llu vertices", (unsigned long long)nVerts);
    if (onDevice && ((uintptr_t)positions12 & 3)) return fail(TBVH_E_INVALID, "tbvh_pose_create_morph: device positions must be 4-byte aligned");
    TBVH_ENTER(c);
    tbvh_pose* p = new (std::nothrow) tbvh_pose;
    if (!p) return fail(TBVH_E_NOMEM, "tbvh_pose_create_morph: out of host memory");
    p->ctx = c; p->kind = kPoseMorph; p->nVerts = nVerts; p->nTargets = nTargets;
    const uint64_t nFloats = ((uint64_t)nTargets + 1) * nVerts * 3;
    if (p->positions.alloc(nFloats) != hipSuccess || p->out.alloc(nVerts) != hipSuccess || p->params.alloc(nTargets ? nTargets : 1) != hipSuccess) {
        destroyPose(p);
        return allocFail("tbvh_pose_create_morph", nFloats * 4 + nVerts * 16 + (nTargets ? nTargets : 1) * 4ull);   // (positions, output, weights)
    }
    int r = makeStaging(p, (uint64_t)nTargets * 4);
    if (!r && (hipMemcpyAsync(p->positions, positions12, nFloats * 4, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream) != hipSuccess ||
               hipMemsetAsync(p->out, 0, nVerts * 16, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess))
        r = fail(TBVH_E_HIP, "tbvh_pose_create_morph: copying the positions failed: %s", hipGetErrorString(hipGetLastError()));
    if (r) { destroyPose(p); return r; }
    c->poses.push_back(p);
    *out = p;
    return 0;
}

int tbvh_pose_set_skin(tbvh_pose* p, const float* mats16, uint32_t nJoints, int onDevice) {
    if (!p || !mats16) return fail(TBVH_E_INVALID, "tbvh_pose_set_skin: null argument");
    if (p->kind != kPoseSkin) return fail(TBVH_E_INVALID, "tbvh_pose_set_skin: a morph pose takes tbvh_pose_set_morph");
    if (nJoints != p->nJoints) return fail(TBVH_E_INVALID, "tbvh_pose_set_skin: %u joint matrices, the pose was created with %u joints", nJoints, p->nJoints);
    if (onDevice && ((uintptr_t)mats16 & 15)) return fail(TBVH_E_INVALID, "tbvh_pose_set_skin: device matrices must be 16-byte aligned");
    tbvh_context* c = p->ctx;
    TBVH_ENTER(c);
    float4* fat = nullptr;
    if (int r = attachedRecords(p, "tbvh_pose_set_skin", &fat)) return r;
    const float* dMats = nullptr;
    if (int r = stageParams(p, mats16, (uint64_t)nJoints * 64, onDevice, &dMats)) return r;
    HIP_TRY(timedBegin(c));
    if (p->shading) {
        launch_pose_skin_normals(p->rest, p->joints, p->weights, (const float4*)dMats, nJoints, p->normals, p->out, p->nOut, p->nVerts, c->status, c->stream);
        updateFatTris(p, fat);
    } else
        launch_pose_skin(p->rest, p->joints, p->weights, (const float4*)dMats, nJoints, p->out, p->nVerts, c->status, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    return 0;
}

int tbvh_pose_set_morph(tbvh_pose* p, const float* weights, uint32_t nTargets, int onDevice) {
    if (!p) return fail(TBVH_E_INVALID, "tbvh_pose_set_morph: null argument");
    if (p->kind != kPoseMorph) return fail(TBVH_E_INVALID, "tbvh_pose_set_morph: a skin pose takes tbvh_pose_set_skin");
    if (nTargets != p->nTargets) return fail(TBVH_E_INVALID, "tbvh_pose_set_morph: %u weights, the pose was created with %u targets", nTargets, p->nTargets);
    if (nTargets && !weights) return fail(TBVH_E_INVALID, "tbvh_pose_set_morph: null weights");
    if (onDevice && ((uintptr_t)weights & 3)) return fail(TBVH_E_INVALID, "tbvh_pose_set_morph: device weights must be 4-byte aligned");
    tbvh_context* c = p->ctx;
    TBVH_ENTER(c);
    float4* fat = nullptr;
    if (int r = attachedRecords(p, "tbvh_pose_set_morph", &fat)) return r;
    const float* dW = nullptr;
    if (int r = stageParams(p, weights, (uint64_t)nTargets * 4, onDevice, &dW)) return r;
    HIP_TRY(timedBegin(c));
    if (p->shading) {
        launch_pose_morph_normals(p->positions, nTargets ? dW : p->params.get(), nTargets, p->normals, p->out, p->nOut, p->nVerts, c->stream);
        updateFatTris(p, fat);
    } else
        launch_pose_morph(p->positions, nTargets ? dW : p->params.get(), nTargets, p->out, p->nVerts, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    return 0;
}

int tbvh_pose_attach_fat_tris(tbvh_pose* p, tbvh_shading* sh, uint32_t slot, const float* normals12, const uint32_t* indices, uint64_t nTris, int onDevice) {
    if (!p || !sh || !normals12) return fail(TBVH_E_INVALID, "tbvh_pose_attach_fat_tris: null argument");
    if (shadingContext(sh) != p->ctx) return fail(TBVH_E_INVALID, "tbvh_pose_attach_fat_tris: the pose and the shading table belong to different contexts");
    if (((uintptr_t)normals12 | (uintptr_t)indices) & 3) return fail(TBVH_E_INVALID, "tbvh_pose_attach_fat_tris: misaligned normals or indices (4 bytes)");
    if (nTris == 0 || nTris >> 32) return fail(TBVH_E_INVALID, "tbvh_pose_attach_fat_tris: %llu triangles", (unsigned long long)nTris);
    if (!indices && p->nVerts != 3 * nTris)
        return fail(TBVH_E_INVALID, "tbvh_pose_attach_fat_tris: %llu vertices for %llu triangles: without indices triangle i has corners 3i .. 3i + 2", (unsigned long long)p->nVerts, (unsigned long long)nTris);
    tbvh_context* c = p->ctx;
    TBVH_ENTER(c);
    float4* tris = nullptr; uint64_t have = 0;
    shadingSlotRecords(sh, slot, &tris, &have);
    if (have != nTris) return fail(TBVH_E_INVALID, "tbvh_pose_attach_fat_tris: slot %u of the shading table holds %llu records, not %llu", slot, (unsigned long long)have, (unsigned long long)nTris);
    if (indices && !onDevice) {   // before anything is allocated
        const uint64_t bad = pose_first_bad_corner(indices, nTris, p->nVerts);
        if (bad != nTris) return fail(TBVH_E_FORMAT, "tbvh_pose_attach_fat_tris: triangle %llu: an index is not a vertex (%llu vertices)", (unsigned long long)bad, (unsigned long long)p->nVerts);
    }
    const uint64_t nFloats = (p->kind == kPoseMorph ? (uint64_t)p->nTargets + 1 : 1) * p->nVerts * 3;
    DevBuf<float> normals; DevBuf<float4> nOut; DevBuf<uint32_t> idx;
    if (normals.alloc(nFloats) != hipSuccess || nOut.alloc(p->nVerts) != hipSuccess || (indices && idx.alloc(3 * nTris) != hipSuccess))
        return allocFail("tbvh_pose_attach_fat_tris", nFloats * 4 + p->nVerts * 16 + (indices ? nTris * 12 : 0));
    const hipMemcpyKind kind = onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_TRY(hipMemcpyAsync(normals, normals12, nFloats * 4, kind, c->stream));
    if (indices) HIP_TRY(hipMemcpyAsync(idx, indices, nTris * 12, kind, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (the caller's arrays are free on return; a pose in flight no longer reads the buffers replaced below)
    p->normals = std::move(normals); p->nOut = std::move(nOut); p->fatIdx = std::move(idx);
    p->shading = sh; p->slot = slot; p->fatTris = nTris;
    return 0;
}

int tbvh_pose_vertices(tbvh_pose* p, const void** dVerts16, uint64_t* nVerts) {
    if (!p || !dVerts16) return fail(TBVH_E_INVALID, "tbvh_pose_vertices: null argument");
    TBVH_LOCK(p->ctx);
    *dVerts16 = p->out.get();
    if (nVerts) *nVerts = p->nVerts;
    return 0;
}

int tbvh_pose_refit(tbvh_pose* p, tbvh_scene* s) {
    if (!p || !s) return fail(TBVH_E_INVALID, "tbvh_pose_refit: null argument");
    if (s->ctx != p->ctx) return fail(TBVH_E_INVALID, "tbvh_pose_refit: the pose and the scene belong to different contexts");
    TBVH_ENTER(p->ctx);
    if (s->meshIdx) {   // a scene made from an indexed mesh: the shared vertices, the indices the scene holds
        tbvh_mesh m;
        m.verts = p->out.get(); m.n_verts = p->nVerts; m.stride_bytes = 16; m.on_device = 1; m.indices = nullptr; m.n_tris = s->meshIdxTris;
        return tbvh_refit_mesh(s, &m);
    }
    if (p->nVerts % 3) return fail(TBVH_E_INVALID, "tbvh_pose_refit: %llu vertices: a scene without an index buffer takes 3 per triangle", (unsigned long long)p->nVerts);
    return tbvh_refit(s, p->out.get(), p->nVerts / 3, 1);
}

int tbvh_pose_download(tbvh_pose* p, void* dst16, uint64_t capVerts) {
    if (!p || !dst16) return fail(TBVH_E_INVALID, "tbvh_pose_download: null argument");
    if (capVerts < p->nVerts) return fail(TBVH_E_INVALID, "tbvh_pose_download: room for %llu vertices, the pose has %llu", (unsigned long long)capVerts, (unsigned long long)p->nVerts);
    tbvh_context* c = p->ctx;
    TBVH_ENTER(c);
    HIP_TRY(hipMemcpyAsync(dst16, p->out, p->nVerts * 16, hipMemcpyDeviceToHost, c->stream));
    return checkStatus(c);   // (synchronizes)
}

void tbvh_pose_free(tbvh_pose* p) {
    if (!p) return;
    tbvh_context* c = p->ctx;
    TBVH_LOCK(c);
    (void)tbvh_capi::setDevice(c);   // (joins the launch lanes)
    hipStreamSynchronize(c->stream);   // (kernels and refits in flight read the pose's buffers)
    for (size_t i = 0; i < c->poses.size(); i++)
        if (c->poses[i] == p) { c->poses.erase(c->poses.begin() + i); break; }
    destroyPose(p);
}

}  // extern "C"
