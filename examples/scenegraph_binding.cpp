// scenegraph_binding.cpp — tinyhip::SceneGraph (include/tiny_hip.h) driven end to end: a root that turns and slides, a child that is an instance and a skinned
// mesh node with its parent as the one joint, one morph weight.  Every verb of the binding is called; what the device holds afterwards must equal, byte for
// byte, what the host twin (tbvh_host_scenegraph_*) computes for the same calls.  Prints "scenegraph binding ok".  Built by __graft_entry__.build() where
// tiny_bvh.h is found (tiny_hip.h includes it).
#include "tiny_bvh.h"
#include "tiny_hip.h"

#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(call) do { int rc_ = (call); if (rc_) { std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, tbvh_last_error()); return 1; } } while (0)

int main() {
    const int32_t parent[2] = {-1, 0};
    const float translation[6] = {0, 0, 0, 1, 2, 3}, rotation[8] = {1, 0, 0, 0, 1, 0, 0, 0}, scale[6] = {1, 1, 1, 1, 1, 1};
    float matrix[32] = {0}, bind[16] = {0};
    for (int n = 0; n < 2; n++) for (int i = 0; i < 4; i++) matrix[16 * n + 5 * i] = 1;
    for (int i = 0; i < 4; i++) bind[5 * i] = 1;
    bind[3] = 0.5f;
    const uint32_t nWeights[2] = {0, 1}, interp[3] = {TBVH_GRAPH_LINEAR, TBVH_GRAPH_LINEAR, TBVH_GRAPH_STEP}, type[3] = {TBVH_GRAPH_VEC3, TBVH_GRAPH_QUAT, TBVH_GRAPH_FLOAT};
    const uint32_t keyOff[4] = {0, 2, 4, 6}, valOff[4] = {0, 6, 14, 16};
    const float times[6] = {0, 1, 0, 1, 0, 1};
    const float values[16] = {0, 0, 0, 4, 0, 0, /* quats w x y z: small turn about y, lerp branch */ 1, 0, 0, 0, 0.9987503f, 0, 0.0499792f, 0, /* weights */ 0.25f, 0.75f};
    const uint32_t chAnim[3] = {0, 0, 1}, chSampler[3] = {0, 1, 2}, chNode[3] = {0, 0, 1}, chTarget[3] = {0, 1, 3};
    const uint32_t instNode[1] = {1}, skinMesh[1] = {1}, jointOff[2] = {0, 1}, jointNode[1] = {0};
    tbvh_scenegraph_desc d;
    std::memset(&d, 0, sizeof d);
    d.n_nodes = 2; d.parent = parent; d.translation = translation; d.rotation = rotation; d.scale = scale; d.matrix = matrix; d.local_transform = matrix; d.n_weights = nWeights;
    d.n_samplers = 3; d.sampler_interpolation = interp; d.sampler_type = type; d.sampler_key_offset = keyOff; d.sampler_value_offset = valOff; d.key_times = times; d.key_values = values;
    d.n_animations = 2; d.n_channels = 3; d.channel_animation = chAnim; d.channel_sampler = chSampler; d.channel_node = chNode; d.channel_target = chTarget;
    d.n_instances = 1; d.node_of_instance = instNode; d.n_skin_uses = 1; d.skin_mesh_node = skinMesh; d.skin_joint_offset = jointOff; d.skin_joint_node = jointNode; d.skin_inverse_bind = bind;

    tbvh_host_scenegraph* host = nullptr;
    CHECK(tbvh_host_scenegraph_create(&d, &host));
    float slide[16] = {1, 0, 0, 0.5f, 0, 1, 0, 0, 0, 0, 1, -2, 0, 0, 0, 1};
    int bad = 0;
    {
        tinyhip::SceneGraph graph(d);
        size_t nInst = 0; uint32_t nJoints = 0, nW = 0;
        const float* dInst = graph.InstanceTransforms(&nInst);
        const float* dJoints = graph.JointMatrices(0, &nJoints);
        const float* dWeights = graph.MorphWeights(1, &nW);
        if (!dInst || !dJoints || !dWeights || nInst != 1 || nJoints != 1 || nW != 1 || !graph.Handle()) { std::fprintf(stderr, "outputs: %zu instances, %u joints, %u weights\n", nInst, nJoints, nW); return 1; }
        auto compare = [&](const char* when) {
            for (int what : {TBVH_GRAPH_TRS, TBVH_GRAPH_LOCAL, TBVH_GRAPH_COMBINED, TBVH_GRAPH_CHANNEL_T, TBVH_GRAPH_CHANNEL_K, TBVH_GRAPH_INSTANCES, TBVH_GRAPH_JOINTS, TBVH_GRAPH_WEIGHTS}) {
                float a[64] = {0}, b[64] = {0};
                graph.Download(what, a, sizeof a);
                if (tbvh_host_scenegraph_download(host, what, b, sizeof b) || std::memcmp(a, b, sizeof a)) { std::fprintf(stderr, "%s: array %d differs from the host twin's\n", when, what); bad++; }
            }
        };
        graph.Advance(0.25f); CHECK(tbvh_host_scenegraph_advance(host, 0.25f)); compare("Advance");
        graph.SetTime(0, 0.5f); graph.Reset(1); graph.AdvanceAnimation(0, 0.125f); graph.AdvanceAnimation(1, 0.625f); graph.UpdateNodes();
        CHECK(tbvh_host_scenegraph_set_time(host, 0, 0.5f)); CHECK(tbvh_host_scenegraph_reset(host, 1)); CHECK(tbvh_host_scenegraph_advance_animation(host, 0, 0.125f));
        CHECK(tbvh_host_scenegraph_advance_animation(host, 1, 0.625f)); CHECK(tbvh_host_scenegraph_update_nodes(host)); compare("SetTime / Reset / AdvanceAnimation / UpdateNodes");
        graph.SetNodeTransform(1, slide); graph.UpdateNodes();
        CHECK(tbvh_host_scenegraph_set_local(host, 1, slide)); CHECK(tbvh_host_scenegraph_update_nodes(host)); compare("SetNodeTransform");
    }
    tbvh_host_scenegraph_free(host);
    if (bad) return 2;
    std::printf("scenegraph binding ok\n");
    return 0;
}
