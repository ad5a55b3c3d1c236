// animated_scene.cpp — the animated frame of the reference's glTF demo (tiny_scene.h, Scene::UpdateSceneGraph: play the animations, walk the node tree, pose the
// skinned meshes, rebuild the TLAS) on the HIP engine with NO host computation per frame, using only the C ABI.  A small scene graph — a turning root, under it a
// skinned tube and its chain of four joints, two of them animated — is made once; per frame one float goes up:
//   tbvh_scenegraph_advance( graph, dt )                        keyframes -> T, R, S -> local and combined matrices -> instance transforms, joint matrices
//   tbvh_pose_set_skin( pose, d_joint_mats, nJoints, 1 )        the joint matrices are read where the graph wrote them
//   tbvh_pose_refit( pose, blas )                               the BLAS follows the posed vertices
//   tbvh_rebuild_tlas_device( tlas, d_instance_mats, 1, .. )    the TLAS follows the instance transforms, likewise from device memory
// and a fixed camera batch is traced.  Prints the hit count per frame.  Builds without the reference: the layouts come from the library's own host builder.
//
//   g++ -O2 -Iinclude examples/animated_scene.cpp -Ltinybvh_amd -ltinybvh_amd -Wl,-rpath,$PWD/tinybvh_amd -o examples/_build/animated_scene
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tinybvh_amd.h"

struct Vec4 { float x, y, z, w; };
struct UInt4 { uint32_t x, y, z, w; };
struct Ray64 { float O[3]; uint32_t mask; float D[3]; uint32_t instIdx; float rD[3]; uint32_t inst; float t, u, v; uint32_t prim; };
struct Instance { float transform[16], invTransform[16]; float aabbMin[3]; uint32_t blasIdx; float aabbMax[3]; uint32_t mask; uint32_t dummy[8]; };
static_assert(sizeof(Ray64) == 64 && sizeof(Instance) == 192, "record sizes of the C ABI");

static float safercp(float x) { return (x > 1e-12f || x < -1e-12f) ? 1.0f / x : (x >= 0 ? 1e30f : -1e30f); }

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, tbvh_last_error()); return 1; } } while (0)

int main() {
    // the tube of examples/skinned_mesh.cpp: RINGS rings of SIDES vertices along y, bound to the two joints a vertex lies between
    const int RINGS = 33, SIDES = 24, JOINTS = 4;
    const float height = 4.0f, radius = 0.5f, segment = height / (JOINTS - 1);
    std::vector<Vec4> rest; std::vector<UInt4> joints; std::vector<Vec4> weights; std::vector<uint32_t> indices;
    for (int r = 0; r < RINGS; r++)
        for (int s = 0; s < SIDES; s++) {
            const float y = height * r / (RINGS - 1), a = 6.2831853f * s / SIDES;
            rest.push_back(Vec4{radius * cosf(a), y, radius * sinf(a), 0});
            int j0 = (int)(y / segment); if (j0 > JOINTS - 2) j0 = JOINTS - 2;
            const float f = y / segment - j0;
            joints.push_back(UInt4{(uint32_t)j0, (uint32_t)j0 + 1, 0, 0});
            weights.push_back(Vec4{1.0f - f, f, 0, 0});
        }
    for (int r = 0; r + 1 < RINGS; r++)
        for (int s = 0; s < SIDES; s++) {
            const uint32_t a = r * SIDES + s, b = r * SIDES + (s + 1) % SIDES, c = a + SIDES, d = b + SIDES;
            const uint32_t quad[6] = {a, b, c, b, d, c};
            indices.insert(indices.end(), quad, quad + 6);
        }
    tbvh_mesh mesh;
    mesh.verts = rest.data(); mesh.n_verts = rest.size(); mesh.stride_bytes = 16; mesh.on_device = 0; mesh.indices = indices.data(); mesh.n_tris = indices.size() / 3;

    // the scene graph: node 0 the root (turns about y), node 1 the tube's mesh node, nodes 2 .. 5 the joints, a chain up the tube; the mesh node comes before its
    // skeleton in the walk, so TBVH_SCENEGRAPH_FRESH_JOINTS asks for this frame's joint transforms (without it the reference's one-frame lag is reproduced)
    const int NODES = 2 + JOINTS;
    const int32_t parent[NODES] = {-1, 0, 0, 2, 3, 4};
    float translation[NODES * 3] = {0}, rotation[NODES * 4] = {0}, scale[NODES * 3], matrix[NODES * 16] = {0}, inverseBind[JOINTS * 16] = {0};
    for (int n = 0; n < NODES; n++) {
        rotation[4 * n] = 1;   // (w x y z)
        for (int i = 0; i < 3; i++) scale[3 * n + i] = 1;
        for (int i = 0; i < 4; i++) matrix[16 * n + 5 * i] = 1;
        if (n >= 3) translation[3 * n + 1] = segment;
    }
    for (int j = 0; j < JOINTS; j++) {
        for (int i = 0; i < 4; i++) inverseBind[16 * j + 5 * i] = 1;
        inverseBind[16 * j + 7] = -segment * j;   // the inverse of the joint's rest transform: down to the origin
    }
    // three LINEAR rotation samplers of three keys: the root about y, joints 2 and 3 about z
    const float halfAngles[3][3] = {{0.0f, 0.4f, 0.0f}, {0.0f, 0.35f, 0.0f}, {0.0f, 0.5f, 0.0f}};
    const int axisOf[3] = {2, 3, 3};   // the quaternion component the sine goes to: y, z, z
    float keyTimes[9], keyValues[36] = {0};
    uint32_t interpolation[3], type[3], keyOffset[4] = {0, 3, 6, 9}, valueOffset[4] = {0, 12, 24, 36};
    for (int s = 0; s < 3; s++) {
        interpolation[s] = TBVH_GRAPH_LINEAR; type[s] = TBVH_GRAPH_QUAT;
        for (int k = 0; k < 3; k++) {
            keyTimes[3 * s + k] = 1.0f * k;
            keyValues[12 * s + 4 * k] = cosf(halfAngles[s][k]);
            keyValues[12 * s + 4 * k + axisOf[s]] = sinf(halfAngles[s][k]);
        }
    }
    const uint32_t chAnim[3] = {0, 0, 0}, chSampler[3] = {0, 1, 2}, chNode[3] = {0, 4, 5}, chTarget[3] = {1, 1, 1};
    const uint32_t instNode[1] = {1}, skinMesh[1] = {1}, jointOffset[2] = {0, JOINTS}, jointNode[JOINTS] = {2, 3, 4, 5};
    tbvh_scenegraph_desc desc;
    memset(&desc, 0, sizeof desc);
    desc.flags = TBVH_SCENEGRAPH_FRESH_JOINTS;
    desc.n_nodes = NODES; desc.parent = parent; desc.translation = translation; desc.rotation = rotation; desc.scale = scale; desc.matrix = matrix; desc.local_transform = matrix;
    desc.n_samplers = 3; desc.sampler_interpolation = interpolation; desc.sampler_type = type; desc.sampler_key_offset = keyOffset; desc.sampler_value_offset = valueOffset;
    desc.key_times = keyTimes; desc.key_values = keyValues;
    desc.n_animations = 1; desc.n_channels = 3; desc.channel_animation = chAnim; desc.channel_sampler = chSampler; desc.channel_node = chNode; desc.channel_target = chTarget;
    desc.n_instances = 1; desc.node_of_instance = instNode;
    desc.n_skin_uses = 1; desc.skin_mesh_node = skinMesh; desc.skin_joint_offset = jointOffset; desc.skin_joint_node = jointNode; desc.skin_inverse_bind = inverseBind;

    tbvh_context* ctx = nullptr;
    CHECK(tbvh_init(0, &ctx));
    tbvh_hostbvh* host = nullptr;
    CHECK(tbvh_host_build_mesh(&mesh, TBVH_LAYOUT_CWBVH, nullptr, &host));
    tbvh_scene* blas = nullptr;
    CHECK(tbvh_upload_host_mesh(ctx, host, &mesh, &blas));
    tbvh_pose* pose = nullptr;
    CHECK(tbvh_pose_create_skin(ctx, rest.data(), rest.size(), &joints[0].x, weights.data(), JOINTS, 0, &pose));
    tbvh_scenegraph* graph = nullptr;
    CHECK(tbvh_scenegraph_create(ctx, &desc, &graph));
    const float* dInstanceMats = nullptr; const float* dJointMats = nullptr; uint64_t nInst = 0; uint32_t nJoints = 0;
    CHECK(tbvh_scenegraph_instance_transforms(graph, &dInstanceMats, &nInst));
    CHECK(tbvh_scenegraph_joint_matrices(graph, 0, &dJointMats, &nJoints));

    // one instance; the BLAS box given to the TLAS rebuild holds every pose of the tube (it bends within height + radius of its foot)
    Instance inst;
    memset(&inst, 0, sizeof inst);
    for (int i = 0; i < 4; i++) inst.transform[5 * i] = inst.invTransform[5 * i] = 1.0f;
    inst.mask = 0xFFFF;
    const float reach = height + radius, bounds[6] = {-reach, -reach, -reach, reach, reach, reach};
    tbvh_hostbvh* tlasHost = nullptr;
    CHECK(tbvh_host_build_tlas(&inst, 1, bounds, 1, &tlasHost));
    tbvh_scene* tlas = nullptr;
    CHECK(tbvh_upload_tlas(ctx, tbvh_host_blob(tlasHost, 0), tbvh_host_blob_count(tlasHost, 0), (const uint32_t*)tbvh_host_blob(tlasHost, 1),
                           tbvh_host_blob_count(tlasHost, 1), &inst, 1, &blas, 1, &tlas));

    // 64 x 64 rays from (0, 2, -8) through a 6 x 6 window at z = 0
    std::vector<Ray64> camera(64 * 64);
    for (int i = 0; i < 64 * 64; i++) {
        Ray64& r = camera[i];
        memset(&r, 0, sizeof r);
        float d[3] = {((i & 63) + 0.5f) / 64.0f * 6.0f - 3.0f, ((i >> 6) + 0.5f) / 64.0f * 6.0f - 3.0f, 8.0f};
        const float l = 1.0f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        r.O[0] = 0.0f; r.O[1] = 2.0f; r.O[2] = -8.0f; r.mask = 0xFFFF;
        for (int a = 0; a < 3; a++) { r.D[a] = d[a] * l; r.rD[a] = safercp(r.D[a]); }
        r.t = 1e30f;
    }

    int first = -1, changed = 0;
    for (int frame = 0; frame < 8; frame++) {
        CHECK(tbvh_scenegraph_advance(graph, frame ? 0.25f : 0.0f));   // the one float of the frame
        CHECK(tbvh_pose_set_skin(pose, dJointMats, nJoints, 1));
        CHECK(tbvh_pose_refit(pose, blas));
        CHECK(tbvh_rebuild_tlas_device(tlas, dInstanceMats, 1, frame ? nullptr : bounds, frame ? 0 : 1));
        std::vector<Ray64> rays = camera;
        CHECK(tbvh_intersect(tlas, rays.data(), rays.size(), sizeof(Ray64)));
        int hits = 0;
        for (const Ray64& r : rays) if (r.t < 1e30f) hits++;
        printf("frame %d: %d of %zu camera rays hit the animated tube\n", frame, hits, rays.size());
        if (frame == 0) first = hits; else if (hits != first) changed++;
    }
    tbvh_scenegraph_free(graph);
    tbvh_pose_free(pose);
    tbvh_free_scene(tlas);
    tbvh_free_scene(blas);
    tbvh_host_free(tlasHost);
    tbvh_host_free(host);
    tbvh_shutdown(ctx);
    if (first <= 0 || changed == 0) { fprintf(stderr, "the tube was not hit, or never moved\n"); return 2; }
    printf("animated scene ok\n");
    return 0;
}
