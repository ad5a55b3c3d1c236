// skinned_mesh.cpp — the animation step of the reference's glTF demo (tiny_scene.h, Node::Update: mesh->SetPose( skin ), then the BLAS is rebuilt
// or refitted) on the HIP engine, using only the C ABI: a small procedural tube skinned to a chain of joints, built once, and per frame
//   tbvh_pose_set_skin( pose, jointMats, nJoints, 0 )   64 bytes per joint go to the device, the vertices are posed there
//   tbvh_pose_refit( pose, blas )                       the BLAS follows them
// under a TLAS that is uploaded once (its instance box holds every frame).  Prints the hit count of a fixed camera batch per frame.
// Builds without the reference: the layouts come from the library's own host builder.
//
//   g++ -O2 -Iinclude examples/skinned_mesh.cpp -Ltinybvh_amd -ltinybvh_amd -Wl,-rpath,$PWD/tinybvh_amd -o examples/_build/skinned_mesh
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tinybvh_amd.h"

struct Vec4 { float x, y, z, w; };
struct UInt4 { uint32_t x, y, z, w; };
struct Mat4 { float cell[16]; };
struct Ray64 { float O[3]; uint32_t mask; float D[3]; uint32_t instIdx; float rD[3]; uint32_t inst; float t, u, v; uint32_t prim; };
struct Instance { float transform[16], invTransform[16]; float aabbMin[3]; uint32_t blasIdx; float aabbMax[3]; uint32_t mask; uint32_t dummy[8]; };
static_assert(sizeof(Ray64) == 64 && sizeof(Instance) == 192, "record sizes of the C ABI");

static float safercp(float x) { return (x > 1e-12f || x < -1e-12f) ? 1.0f / x : (x >= 0 ? 1e30f : -1e30f); }

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, tbvh_last_error()); return 1; } } while (0)

// joint j of the chain turns about the z axis through (0, j * segment, 0); joints above the first two stay where they are
static Mat4 jointMatrix(float pivotY, float angle) {
    const float c = cosf(angle), s = sinf(angle);
    Mat4 m = {{c, -s, 0, s * pivotY, s, c, 0, pivotY - c * pivotY, 0, 0, 1, 0, 0, 0, 0, 1}};
    return m;
}

int main() {
    // a tube along y: RINGS rings of SIDES vertices, two triangles per quad, indexed (every vertex is posed once)
    const int RINGS = 33, SIDES = 24, JOINTS = 4;
    const float height = 4.0f, radius = 0.5f, segment = height / (JOINTS - 1);
    std::vector<Vec4> rest; std::vector<UInt4> joints; std::vector<Vec4> weights; std::vector<uint32_t> indices;
    for (int r = 0; r < RINGS; r++)
        for (int s = 0; s < SIDES; s++) {
            const float y = height * r / (RINGS - 1), a = 6.2831853f * s / SIDES;
            rest.push_back(Vec4{radius * cosf(a), y, radius * sinf(a), 0});
            // the two joints the vertex lies between, weighted by distance
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

    tbvh_context* ctx = nullptr;
    CHECK(tbvh_init(0, &ctx));
    tbvh_hostbvh* host = nullptr;
    CHECK(tbvh_host_build_mesh(&mesh, TBVH_LAYOUT_CWBVH, nullptr, &host));
    tbvh_scene* blas = nullptr;
    CHECK(tbvh_upload_host_mesh(ctx, host, &mesh, &blas));
    tbvh_pose* pose = nullptr;
    CHECK(tbvh_pose_create_skin(ctx, rest.data(), rest.size(), &joints[0].x, weights.data(), JOINTS, 0, &pose));

    // one instance, identity; its box holds every pose of the tube (it bends within height + radius of the origin in x and y)
    Instance inst;
    memset(&inst, 0, sizeof inst);
    for (int i = 0; i < 4; i++) inst.transform[5 * i] = inst.invTransform[5 * i] = 1.0f;
    inst.mask = 0xFFFF;
    const float reach = height + radius, bounds[6] = {-reach, -reach, -radius, reach, reach, radius};
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
    for (int frame = 0; frame < 6; frame++) {
        // joints 0 and 1 stay; joints 2 and 3 swing: the upper half of the tube bends over
        Mat4 mats[JOINTS];
        for (int j = 0; j < JOINTS; j++) mats[j] = jointMatrix(j * segment, 0.0f);
        mats[2] = jointMatrix(2 * segment, 0.25f * frame);
        mats[3] = jointMatrix(2 * segment, 0.45f * frame);
        CHECK(tbvh_pose_set_skin(pose, mats[0].cell, JOINTS, 0));
        CHECK(tbvh_pose_refit(pose, blas));
        std::vector<Ray64> rays = camera;
        CHECK(tbvh_intersect(tlas, rays.data(), rays.size(), sizeof(Ray64)));
        int hits = 0;
        for (const Ray64& r : rays) if (r.t < 1e30f) hits++;
        printf("frame %d: %d of %zu camera rays hit the skinned tube\n", frame, hits, rays.size());
        if (frame == 0) first = hits; else if (hits != first) changed++;
    }
    tbvh_pose_free(pose);
    tbvh_free_scene(tlas);
    tbvh_free_scene(blas);
    tbvh_host_free(tlasHost);
    tbvh_host_free(host);
    tbvh_shutdown(ctx);
    if (first <= 0 || changed == 0) { fprintf(stderr, "the tube was not hit, or never moved\n"); return 2; }
    printf("skinned mesh ok\n");
    return 0;
}
