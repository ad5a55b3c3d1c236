// viewer_frame.cpp — a frame of the reference's CPU viewer (tiny_bvh_gltf.cpp: WorkerThread, Trace, SampleSky) from the camera to the pixels without leaving
// the device, using only the C ABI:
//   tbvh_sky_create( ctx, pixels, w, h, .. )                         SkyDome::pixels, once
//   tbvh_viewer_create( ctx, 256, 256, &viewer )                     the frame's buffers, once
//   tbvh_viewer_render( viewer, tlas, shading, sky, &cam, &params, &stats )   generate, { trace, shade } x rounds, light, pack
//   tbvh_viewer_read_pixels( viewer, pixels )                        0x00BBGGRR, as the reference's window buffer
// The alpha loop of examples/shaded_hits.cpp — a counter read back per round, the lighting on the host — is gone: the rays that continue are compacted
// into a queue on the device.  The scene is the one of shaded_hits.cpp: a quad with a checker texture whose dark squares are masked, in front of an
// untextured pyramid, both under one TLAS.  Writes viewer_frame.ppm and checks that the quad is seen, that the pyramid and the sky show through its
// holes and that the loop ends after its second round.
// Builds without the reference: the layouts come from the library's own host builder.
//
//   g++ -O2 -Iinclude examples/viewer_frame.cpp -Ltinybvh_amd -ltinybvh_amd -Wl,-rpath,$PWD/tinybvh_amd -o examples/_build/viewer_frame
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tinybvh_amd.h"

struct Vec4 { float x, y, z, w; };
struct Ray64 { float O[3]; uint32_t mask; float D[3]; uint32_t instIdx; float rD[3]; uint32_t inst; float t, u, v; uint32_t prim; };
struct Instance { float transform[16], invTransform[16]; float aabbMin[3]; uint32_t blasIdx; float aabbMax[3]; uint32_t mask; uint32_t dummy[8]; };
// tinyscene::FatTri
struct FatTri {
    float u0, u1, u2; int ltriIdx; float v0, v1, v2; uint32_t material;
    float vN0[3], Nx, vN1[3], Ny, vN2[3], Nz;
    float vertex0[3], u0_2, vertex1[3], u1_2, vertex2[3], u2_2;
    float T[3], area, B[3], invArea, alpha[3], LOD, v0_2, v1_2, v2_2, dummy4;
};
struct Shaded { float albedo[3], alpha, N[3]; uint32_t material; float iN[3]; uint32_t texel; };
static_assert(sizeof(Ray64) == 64 && sizeof(Instance) == 192 && sizeof(FatTri) == 192 && sizeof(Shaded) == 48, "record sizes of the C ABI");

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, tbvh_last_error()); return 1; } } while (0)

// flat-shaded FatTris for a triangle soup: every vertex normal is the face normal, UVs are given per corner
static std::vector<FatTri> fatTris(const std::vector<Vec4>& v, const std::vector<float>& uv, uint32_t material) {
    std::vector<FatTri> out(v.size() / 3);
    for (size_t i = 0; i < out.size(); i++) {
        FatTri& f = out[i];
        memset(&f, 0, sizeof f);
        const Vec4 &a = v[3 * i], &b = v[3 * i + 1], &c = v[3 * i + 2];
        const float e1[3] = {b.x - a.x, b.y - a.y, b.z - a.z}, e2[3] = {c.x - a.x, c.y - a.y, c.z - a.z};
        float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const float l = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        for (float& x : n) x /= l;
        f.ltriIdx = -1; f.material = material;
        f.Nx = n[0]; f.Ny = n[1]; f.Nz = n[2];
        for (int k = 0; k < 3; k++) f.vN0[k] = f.vN1[k] = f.vN2[k] = n[k];
        const Vec4* p[3] = {&a, &b, &c};
        float* dst[3] = {f.vertex0, f.vertex1, f.vertex2};
        for (int k = 0; k < 3; k++) { dst[k][0] = p[k]->x; dst[k][1] = p[k]->y; dst[k][2] = p[k]->z; }
        if (!uv.empty()) {
            f.u0 = uv[6 * i]; f.v0 = uv[6 * i + 1]; f.u1 = uv[6 * i + 2]; f.v1 = uv[6 * i + 3]; f.u2 = uv[6 * i + 4]; f.v2 = uv[6 * i + 5];
        }
    }
    return out;
}

int main() {
    // slot 0: a quad in the plane z = 0, UVs its corners; slot 1: a four-sided pyramid behind it
    const std::vector<Vec4> quad = {{-2, -2, 0, 0}, {2, -2, 0, 0}, {2, 2, 0, 0}, {-2, -2, 0, 0}, {2, 2, 0, 0}, {-2, 2, 0, 0}};
    const std::vector<float> quadUV = {0, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1};
    const Vec4 apex = {0, 0, 1.2f, 0}, c0 = {-1.5f, -1.5f, 3, 0}, c1 = {1.5f, -1.5f, 3, 0}, c2 = {1.5f, 1.5f, 3, 0}, c3 = {-1.5f, 1.5f, 3, 0};
    const std::vector<Vec4> pyramid = {apex, c1, c0, apex, c2, c1, apex, c3, c2, apex, c0, c3};
    // a 16 x 16 checker: light squares opaque, the nearly black squares masked
    const uint32_t W = 16, H = 16;
    std::vector<uint32_t> texels(W * H);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) texels[x + y * W] = ((x / 2 + y / 2) & 1) ? 0xFF010101u : 0xFFE0C040u;   // (x = red in the low byte; x + y + z <= 5: masked for tiny_bvh_gltf.cpp)
    const tbvh_alpha_texture textures[1] = {{texels.data(), W, H}};
    const tbvh_material materials[2] = {{{1, 1, 1}, 0, TBVH_OMM_NO_TEXTURE}, {{0.2f, 0.5f, 0.9f}, TBVH_OMM_NO_TEXTURE, TBVH_OMM_NO_TEXTURE}};
    const std::vector<FatTri> fatQuad = fatTris(quad, quadUV, 0), fatPyramid = fatTris(pyramid, {}, 1);

    tbvh_context* ctx = nullptr;
    CHECK(tbvh_init(0, &ctx));
    tbvh_hostbvh* host[2] = {nullptr, nullptr};
    tbvh_scene* blas[2] = {nullptr, nullptr};
    CHECK(tbvh_host_build(quad.data(), quad.size() / 3, TBVH_LAYOUT_CWBVH, nullptr, &host[0]));
    CHECK(tbvh_host_build(pyramid.data(), pyramid.size() / 3, TBVH_LAYOUT_CWBVH, nullptr, &host[1]));
    CHECK(tbvh_upload_host(ctx, host[0], quad.data(), quad.size() / 3, &blas[0]));
    CHECK(tbvh_upload_host(ctx, host[1], pyramid.data(), pyramid.size() / 3, &blas[1]));
    Instance inst[2];
    memset(inst, 0, sizeof inst);
    for (int k = 0; k < 2; k++) {
        for (int i = 0; i < 4; i++) inst[k].transform[5 * i] = inst[k].invTransform[5 * i] = 1.0f;
        inst[k].blasIdx = (uint32_t)k; inst[k].mask = 0xFFFF;
    }
    const float bounds[12] = {-2, -2, 0, 2, 2, 0, -1.5f, -1.5f, 1.2f, 1.5f, 1.5f, 3};
    tbvh_hostbvh* tlasHost = nullptr;
    CHECK(tbvh_host_build_tlas(inst, 2, bounds, 2, &tlasHost));
    tbvh_scene* tlas = nullptr;
    CHECK(tbvh_upload_tlas(ctx, tbvh_host_blob(tlasHost, 0), tbvh_host_blob_count(tlasHost, 0), (const uint32_t*)tbvh_host_blob(tlasHost, 1),
                           tbvh_host_blob_count(tlasHost, 1), inst, 2, blas, 2, &tlas));
    tbvh_shading* shading = nullptr;
    CHECK(tbvh_shading_create(ctx, materials, 2, textures, 1, 0, &shading));
    CHECK(tbvh_shading_set_fat_tris(shading, 0, fatQuad.data(), fatQuad.size(), 0));
    CHECK(tbvh_shading_set_fat_tris(shading, 1, fatPyramid.data(), fatPyramid.size(), 0));

    // a small sky: blue above, warm at the horizon, dark below (3 floats per texel, as SkyDome::pixels after Load)
    const uint32_t SW = 16, SH = 8;
    std::vector<float> skyPixels(3 * SW * SH);
    for (uint32_t y = 0; y < SH; y++)
        for (uint32_t x = 0; x < SW; x++) {
            const float up = 1.0f - (y + 0.5f) / SH;
            float* t = &skyPixels[3 * (x + y * SW)];
            t[0] = 0.9f * up + 0.1f; t[1] = 0.5f * up + 0.2f; t[2] = 0.3f + 0.05f * (x & 1);   // (SampleSky returns the texel as z, y, x)
        }
    tbvh_sky* sky = nullptr;
    CHECK(tbvh_sky_create(ctx, skyPixels.data(), SW, SH, 0, &sky));

    // the view pyramid: the eye at (0.3, 0.2, -6), the corners of a 5 x 5 window at z = 0 (p1 top left, p2 top right, p3 bottom left)
    const uint32_t S = 256;
    const size_t n = (size_t)S * S;
    const tbvh_camera cam = {{0.3f, 0.2f, -6.0f}, {-2.5f, 2.5f, 0}, {2.5f, 2.5f, 0}, {-2.5f, -2.5f, 0}, S, S, 1, 1};
    tbvh_viewer* viewer = nullptr;
    CHECK(tbvh_viewer_create(ctx, S, S, &viewer));
    tbvh_viewer_params params;
    memset(&params, 0, sizeof params);
    params.mode = TBVH_VIEWER_GLTF;
    params.light_dir[0] = -0.3f; params.light_dir[1] = 0.5f; params.light_dir[2] = -0.81f;
    tbvh_viewer_stats stats;
    CHECK(tbvh_viewer_render(viewer, tlas, shading, sky, &cam, &params, &stats));
    std::vector<uint32_t> pixels(n);
    CHECK(tbvh_viewer_read_pixels(viewer, pixels.data()));
    std::vector<Ray64> rays(n);
    void* dRays = nullptr;
    CHECK(tbvh_viewer_rays(viewer, &dRays));
    CHECK(tbvh_copy_from_device(ctx, rays.data(), dRays, n * sizeof(Ray64)));
    for (int r = 0; r < 8 && stats.rays[r]; r++) printf("round %d: %llu rays traced\n", r, (unsigned long long)stats.rays[r]);
    printf("frame: %.3f ms on the device\n", stats.frame_ms);

    size_t onQuad = 0, onPyramid = 0, skyPixelsSeen = 0, black = 0;
    FILE* f = fopen("viewer_frame.ppm", "wb");
    if (!f) { perror("viewer_frame.ppm"); return 1; }
    fprintf(f, "P6\n%u %u\n255\n", S, S);
    for (size_t i = 0; i < n; i++) {
        const unsigned char px[3] = {(unsigned char)(pixels[i] & 255), (unsigned char)((pixels[i] >> 8) & 255), (unsigned char)((pixels[i] >> 16) & 255)};
        fwrite(px, 1, 3, f);
        if (!(rays[i].t < 10000.f)) skyPixelsSeen++;
        else (rays[i].inst == 0 ? onQuad : onPyramid)++;
        if (!pixels[i]) black++;
    }
    fclose(f);
    printf("%zu pixels on the quad, %zu on the pyramid, %zu sky\n", onQuad, onPyramid, skyPixelsSeen);

    tbvh_viewer_destroy(viewer);
    tbvh_sky_free(sky);
    tbvh_shading_free(shading);
    tbvh_free_scene(tlas);
    for (int k = 0; k < 2; k++) { tbvh_free_scene(blas[k]); tbvh_host_free(host[k]); }
    tbvh_host_free(tlasHost);
    tbvh_shutdown(ctx);
    // the quad covers 4 / 5 of the window in each direction, half of its squares are holes; behind the holes the pyramid or the sky; a ray crosses the quad
    // once: round 1 traces the rays that went through a hole, round 2 has nothing to do
    if (onQuad < n / 5 || onPyramid < n / 50 || skyPixelsSeen < n / 10 || stats.rays[0] != n || stats.rays[1] < n / 5 || stats.rays[2] || black > n / 100) {
        fprintf(stderr, "unexpected picture\n");
        return 2;
    }
    printf("viewer frame ok\n");
    return 0;
}
