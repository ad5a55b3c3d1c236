// scenegraph_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's Scene::UpdateAnimation / Animation::Update / Channel::Update / Sampler::Sample*,
// Node::Update and Node::UpdateTransformFromTRS (tiny_scene.h) behind a C interface that takes the library's tbvh_scenegraph_desc.
//
// Compiled at test time (tests/scenegraph_lib.py: compile_ref_shim) from $TBVH_REFERENCE with the flags of oracle/Makefile plus -fno-access-control
// (Animation::Sampler and Channel are private nested classes, Node::instanceID is protected), into the pytest temp dir; nothing of the reference is copied
// into the repository.  The `#elif` temp copy and the vector types are those of tests/pose_ref_shim.cpp.  Scene's pools are static, so there is ONE graph
// at a time: sgref_create replaces it.  The pools are filled by hand: every instance's node and every skin use's mesh node gets a one-triangle mesh of
// its own with geomChanged = false and a built dynamicBVH, so that Node::Update runs unmodified (it poses the mesh, and updates the instance); skins get
// three zero-weight vertices, nodes with weights a pose per weight.  sgref_advance is UpdateSceneGraph's two loops without the TLAS build.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#define sprintf_s(buf, ...) snprintf((buf), sizeof(buf), __VA_ARGS__)
#define strcat_s(dst, src) strncat((dst), (src), sizeof(dst) - strlen(dst) - 1)

#define TINYBVH_IMPLEMENTATION
#include "tiny_bvh.h"
#define TINYSCENE_USE_CUSTOM_VECTOR_TYPES
namespace tinyscene {
using ts_int2 = tinybvh::bvhint2;
using ts_int3 = tinybvh::bvhint3;
using ts_uint2 = tinybvh::bvhuint2;
using ts_uint3 = tinybvh::bvhuint3;
using ts_uint4 = tinybvh::bvhuint4;
using ts_vec2 = tinybvh::bvhvec2;
using ts_vec3 = tinybvh::bvhvec3;
using ts_vec4 = tinybvh::bvhvec4;
using ts_mat4 = tinybvh::bvhmat4;
}  // namespace tinyscene
#define TINYSCENE_IMPLEMENTATION
#include "tiny_scene.h"

#include "tinybvh_amd.h"   // (the descriptor and the download codes only)

using namespace tinybvh;
using namespace tinyscene;

namespace {

std::vector<uint32_t> g_instNode, g_useOff;
std::vector<uint32_t> g_wOff;

template <class T>
T* zeroed() { return (T*)calloc(1, sizeof(T)); }

int newMesh(uint32_t nWeights, bool skinned) {
    Mesh* mesh = new Mesh();
    mesh->ID = (int)Scene::meshPool.size();
    mesh->vertices.resize(3);
    mesh->vertices[0] = bvhvec4(0, 0, 0, 0); mesh->vertices[1] = bvhvec4(1, 0, 0, 0); mesh->vertices[2] = bvhvec4(0, 1, 0, 0);
    mesh->triangles.resize(1);
    if (skinned) {
        mesh->joints.resize(3);
        mesh->weights.resize(3);
        std::memset((void*)mesh->joints.data(), 0, 3 * sizeof(bvhuint4));
        std::memset((void*)mesh->weights.data(), 0, 3 * sizeof(bvhvec4));
    }
    if (nWeights) {
        mesh->poses.resize(nWeights + 1);
        for (auto& p : mesh->poses) {
            p.positions.resize(3); p.normals.resize(3);
            for (int i = 0; i < 3; i++) p.positions[i] = bvhvec3(mesh->vertices[i].x, mesh->vertices[i].y, mesh->vertices[i].z), p.normals[i] = bvhvec3(0, 0, 1);
        }
    }
    mesh->blas.dynamicBVH = new BVH();
    mesh->blas.dynamicBVH->Build((bvhvec4*)mesh->vertices.data(), 1);
    mesh->geomChanged = false;
    Scene::meshPool.push_back(mesh);
    return mesh->ID;
}

}  // namespace

extern "C" {

int sgref_create(const tbvh_scenegraph_desc* d) {
    Scene::rootNodes.clear(); Scene::nodePool.clear(); Scene::meshPool.clear(); Scene::instPool.clear(); Scene::skins.clear(); Scene::animations.clear();   // (the old graph leaks)
    const uint32_t N = (uint32_t)d->n_nodes;
    g_wOff.assign(N + 1, 0);
    for (uint32_t n = 0; n < N; n++) {
        Node* node = new Node();
        node->ID = (int)n;
        node->translation = bvhvec3(d->translation[3 * n], d->translation[3 * n + 1], d->translation[3 * n + 2]);
        node->rotation = ts_quat(d->rotation[4 * n], d->rotation[4 * n + 1], d->rotation[4 * n + 2], d->rotation[4 * n + 3]);
        node->scale = bvhvec3(d->scale[3 * n], d->scale[3 * n + 1], d->scale[3 * n + 2]);
        std::memcpy(&node->matrix, d->matrix + 16 * (size_t)n, 64);
        std::memcpy(&node->localTransform, d->local_transform + 16 * (size_t)n, 64);
        const uint32_t nw = d->n_weights ? d->n_weights[n] : 0;
        g_wOff[n + 1] = g_wOff[n] + nw;
        node->weights.resize(nw);
        for (uint32_t i = 0; i < nw; i++) node->weights[i] = d->weights ? d->weights[g_wOff[n] + i] : 0.f;
        Scene::nodePool.push_back(node);
    }
    // children and roots: in visit_order's order of appearance, or by increasing index
    for (uint32_t i = 0; i < N; i++) {
        const uint32_t n = d->visit_order ? d->visit_order[i] : i;
        if (d->parent[n] < 0) Scene::rootNodes.push_back((int)n);
        else Scene::nodePool[d->parent[n]]->childIdx.push_back((int)n);
    }
    g_instNode.assign(d->node_of_instance, d->node_of_instance + d->n_instances);
    for (uint32_t i = 0; i < d->n_instances; i++) {
        Node* node = Scene::nodePool[d->node_of_instance[i]];
        if (node->meshID < 0) node->meshID = newMesh((uint32_t)node->weights.size(), false);
    }
    g_useOff.assign(1, 0);
    for (uint32_t u = 0; u < d->n_skin_uses; u++) {
        Node* node = Scene::nodePool[d->skin_mesh_node[u]];
        if (node->meshID >= 0) {   // (an instance's plain mesh: it needs the skinning arrays)
            Mesh* mesh = Scene::meshPool[node->meshID];
            mesh->joints.resize(3); mesh->weights.resize(3);
            std::memset((void*)mesh->joints.data(), 0, 3 * sizeof(bvhuint4));
            std::memset((void*)mesh->weights.data(), 0, 3 * sizeof(bvhvec4));
        } else
            node->meshID = newMesh((uint32_t)node->weights.size(), true);
        Skin* skin = zeroed<Skin>();
        new (&skin->name) std::string();
        new (&skin->inverseBindMatrices) std::vector<bvhmat4>();
        new (&skin->jointMat) std::vector<bvhmat4>();
        new (&skin->joints) std::vector<int>();
        const uint32_t j0 = d->skin_joint_offset[u], j1 = d->skin_joint_offset[u + 1];
        skin->joints.assign(d->skin_joint_node + j0, d->skin_joint_node + j1);
        skin->inverseBindMatrices.resize(j1 - j0);
        std::memcpy((void*)skin->inverseBindMatrices.data(), d->skin_inverse_bind + 16 * (size_t)j0, (size_t)(j1 - j0) * 64);
        skin->jointMat.resize(j1 - j0);
        node->skinID = (int)Scene::skins.size();
        Scene::skins.push_back(skin);
        g_useOff.push_back(j1);
    }
    // every animation holds the whole sampler list, so that a channel's samplerIdx is the descriptor's
    std::vector<Animation::Sampler*> samplers;
    for (uint32_t s = 0; s < d->n_samplers; s++) {
        Animation::Sampler* sm = zeroed<Animation::Sampler>();
        new (&sm->t) std::vector<float>();
        new (&sm->vec3Key) std::vector<bvhvec3>();
        new (&sm->vec4Key) std::vector<ts_quat>();
        new (&sm->floatKey) std::vector<float>();
        sm->interpolation = (int)d->sampler_interpolation[s];
        sm->t.assign(d->key_times + d->sampler_key_offset[s], d->key_times + d->sampler_key_offset[s + 1]);
        const float* v = d->key_values + d->sampler_value_offset[s];
        const uint32_t nv = d->sampler_value_offset[s + 1] - d->sampler_value_offset[s];
        if (d->sampler_type[s] == TBVH_GRAPH_VEC3) for (uint32_t i = 0; i + 2 < nv; i += 3) sm->vec3Key.push_back(bvhvec3(v[i], v[i + 1], v[i + 2]));
        else if (d->sampler_type[s] == TBVH_GRAPH_QUAT) for (uint32_t i = 0; i + 3 < nv; i += 4) sm->vec4Key.push_back(ts_quat(v[i], v[i + 1], v[i + 2], v[i + 3]));
        else sm->floatKey.assign(v, v + nv);
        samplers.push_back(sm);
    }
    for (uint32_t a = 0; a < d->n_animations; a++) {
        Animation* an = zeroed<Animation>();
        new (&an->sampler) std::vector<Animation::Sampler*>(samplers);
        new (&an->channel) std::vector<Animation::Channel*>();
        Scene::animations.push_back(an);
    }
    for (uint32_t c = 0; c < d->n_channels; c++) {
        Animation::Channel* ch = zeroed<Animation::Channel>();
        ch->samplerIdx = (int)d->channel_sampler[c]; ch->nodeIdx = (int)d->channel_node[c]; ch->target = (int)d->channel_target[c]; ch->t = 0; ch->k = 0;
        Scene::animations[d->channel_animation[c]]->channel.push_back(ch);
    }
    return 0;
}

void sgref_update_nodes() {
    for (int nodeIdx : Scene::rootNodes) {
        ts_mat4 T;
        Scene::nodePool[nodeIdx]->Update(T);
    }
}
void sgref_advance_animation(uint32_t a, float dt) { Scene::UpdateAnimation((int)a, dt); }
void sgref_advance(float dt) {
    for (int s = Scene::AnimationCount(), i = 0; i < s; i++) Scene::UpdateAnimation(i, dt);
    sgref_update_nodes();
}
void sgref_set_time(uint32_t a, float t) { Scene::animations[a]->SetTime(t); }
void sgref_reset(uint32_t a) { Scene::ResetAnimation((int)a); }
void sgref_set_local(uint32_t node, const float* m) { bvhmat4 M; std::memcpy(&M, m, 64); Scene::SetNodeTransform((int)node, M); }

// the library's download codes (TBVH_GRAPH_*); dst is large enough
int sgref_download(int what, void* dst) {
    float* f = (float*)dst;
    const size_t N = Scene::nodePool.size();
    switch (what) {
    case TBVH_GRAPH_TRS:
        for (size_t n = 0; n < N; n++) {
            const Node* nd = Scene::nodePool[n];
            const float v[10] = {nd->translation.x, nd->translation.y, nd->translation.z, nd->rotation.w, nd->rotation.x, nd->rotation.y, nd->rotation.z, nd->scale.x, nd->scale.y, nd->scale.z};
            std::memcpy(f + 10 * n, v, 40);
        }
        return 0;
    case TBVH_GRAPH_LOCAL: for (size_t n = 0; n < N; n++) std::memcpy(f + 16 * n, &Scene::nodePool[n]->localTransform, 64); return 0;
    case TBVH_GRAPH_COMBINED: for (size_t n = 0; n < N; n++) std::memcpy(f + 16 * n, &Scene::nodePool[n]->combinedTransform, 64); return 0;
    case TBVH_GRAPH_CHANNEL_T: case TBVH_GRAPH_CHANNEL_K: {
        size_t c = 0;
        for (Animation* a : Scene::animations)
            for (Animation::Channel* ch : a->channel) {
                if (what == TBVH_GRAPH_CHANNEL_T) f[c++] = ch->t; else ((int32_t*)dst)[c++] = ch->k;
            }
        return 0;
    }
    case TBVH_GRAPH_INSTANCES:
        for (size_t i = 0; i < g_instNode.size(); i++) {
            const int id = Scene::nodePool[g_instNode[i]]->instanceID;
            if (id < 0) return -1;   // (no walk yet)
            std::memcpy(f + 16 * i, &Scene::instPool[id].transform, 64);
        }
        return 0;
    case TBVH_GRAPH_JOINTS:
        for (size_t u = 0; u < Scene::skins.size(); u++) std::memcpy(f + 16 * (size_t)g_useOff[u], Scene::skins[u]->jointMat.data(), (size_t)(g_useOff[u + 1] - g_useOff[u]) * 64);
        return 0;
    case TBVH_GRAPH_WEIGHTS:
        for (size_t n = 0; n < N; n++) if (g_wOff[n + 1] > g_wOff[n]) std::memcpy(f + g_wOff[n], Scene::nodePool[n]->weights.data(), (size_t)(g_wOff[n + 1] - g_wOff[n]) * 4);
        return 0;
    }
    return -1;
}

// Node::UpdateTransformFromTRS as the glTF loader runs it on a node that gives T, R, S or a matrix: trs = translation, rotation (w x y z), scale
void sgref_local_from_trs(const float* trs, const float* matrix, float* local) {
    Node n;
    n.translation = bvhvec3(trs[0], trs[1], trs[2]); n.rotation = ts_quat(trs[3], trs[4], trs[5], trs[6]); n.scale = bvhvec3(trs[7], trs[8], trs[9]);
    std::memcpy(&n.matrix, matrix, 64);
    n.UpdateTransformFromTRS();
    std::memcpy(local, &n.localTransform, 64);
}

// pieces, for checks of one operation at a time
void sgref_mul(const float* a, const float* b, float* r) { bvhmat4 A, B; std::memcpy(&A, a, 64); std::memcpy(&B, b, 64); const bvhmat4 R = A * B; std::memcpy(r, &R, 64); }
void sgref_invert(const float* a, float* r) { bvhmat4 A; std::memcpy(&A, a, 64); ts_invert(A); std::memcpy(r, &A, 64); }
// the normalised quaternion SampleQuat's LINEAR case returns for keys a, b (w x y z) at f
void sgref_slerp(const float* a, const float* b, float f, float* r) {
    ts_quat q = ts_quat::slerp(ts_quat(a[0], a[1], a[2], a[3]), ts_quat(b[0], b[1], b[2], b[3]), f);
    q.ts_normalize();
    r[0] = q.w; r[1] = q.x; r[2] = q.y; r[3] = q.z;
}

}  // extern "C"
