// shaded_hits.cpp — the first thing every renderer of the reference does with a hit (GetShadingData: hit -> instance -> FatTri -> material -> texel) on the
// HIP engine, using only the C ABI, with everything between the camera rays and the pixel on the device:
//   tbvh_intersect_device( tlas, rays )                              the trace
//   tbvh_shade_hits_device( shading, tlas, rays, .., out48 )         albedo + alpha, N, iN per ray
//   tbvh_shade_continue_device( ctx, rays, .., out48, .., counter )  rays that hit a transparent texel step on (O = I + 1e-4 D, t reset) ...
// ... and are traced again, at most 8 rounds, as tiny_bvh_gltf.cpp:140-150 loops.  The scene: a quad with a checker texture whose dark squares are
// transparent, in front of an untextured pyramid, both under one TLAS.  Writes shaded_hits.ppm (N.L shading of the albedo) and checks that the quad is
// seen, that the pyramid shows through its holes and that the loop ends before its eighth round.
// Builds without the reference: the layouts come from the library's own host builder.
//
//   g++ -O2 -Iinclude examples/shaded_hits.cpp -Ltinybvh_amd -ltinybvh_amd -Wl,-rpath,$PWD/tinybvh_amd -o examples/_build/shaded_hits
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

static float safercp(float x) { return (x > 1e-12f || x < -1e-12f) ? 1.0f / x : (x >= 0 ? 1e30f : -1e30f); }

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
    // a 16 x 16 checker: light squares opaque, dark squares transparent (alpha 0)
    const uint32_t W = 16, H = 16;
    std::vector<uint32_t> texels(W * H);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) texels[x + y * W] = ((x / 2 + y / 2) & 1) ? 0x00202020u : 0xFFE0C040u;   // (x = red in the low byte)
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

    // 256 x 256 rays from (0.3, 0.2, -6) through a 5 x 5 window at z = 0
    const int S = 256;
    const size_t n = (size_t)S * S;
    std::vector<Ray64> rays(n);
    for (size_t i = 0; i < n; i++) {
        Ray64& r = rays[i];
        memset(&r, 0, sizeof r);
        const float O[3] = {0.3f, 0.2f, -6.0f};
        float d[3] = {((i % S) + 0.5f) / S * 5.0f - 2.5f - O[0], 2.5f - ((i / S) + 0.5f) / S * 5.0f - O[1], -O[2]};
        const float l = 1.0f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        r.mask = 0xFFFF;
        for (int a = 0; a < 3; a++) { r.O[a] = O[a]; r.D[a] = d[a] * l; r.rD[a] = safercp(r.D[a]); }
        r.t = 1e30f;
    }
    void *dRays = nullptr, *dOut = nullptr, *dCount = nullptr;
    CHECK(tbvh_device_malloc(ctx, n * sizeof(Ray64), &dRays));
    CHECK(tbvh_device_malloc(ctx, n * sizeof(Shaded), &dOut));
    CHECK(tbvh_device_malloc(ctx, 8, &dCount));
    CHECK(tbvh_copy_to_device(ctx, dRays, rays.data(), n * sizeof(Ray64)));

    // the alpha-continue loop: trace, shade, step the transparent hits on; only the 8-byte counter comes back per round
    int rounds = 0;
    unsigned long long stepped = 0, total = 0;
    for (; rounds < 8; rounds++) {
        const unsigned long long zero = 0;
        CHECK(tbvh_copy_to_device(ctx, dCount, &zero, 8));
        CHECK(tbvh_intersect_device(tlas, dRays, n));
        CHECK(tbvh_shade_hits_device(shading, tlas, dRays, n, sizeof(Ray64), dOut));
        CHECK(tbvh_shade_continue_device(ctx, dRays, sizeof(Ray64), dOut, n, (unsigned long long*)dCount));
        CHECK(tbvh_copy_from_device(ctx, &stepped, dCount, 8));
        printf("round %d: %llu rays stepped through a transparent texel\n", rounds, stepped);
        total += stepped;
        if (!stepped) break;
    }
    std::vector<Shaded> out(n);
    CHECK(tbvh_copy_from_device(ctx, out.data(), dOut, n * sizeof(Shaded)));

    size_t onQuad = 0, onPyramid = 0, sky = 0, transparentLeft = 0;
    FILE* f = fopen("shaded_hits.ppm", "wb");
    if (!f) { perror("shaded_hits.ppm"); return 1; }
    fprintf(f, "P6\n%d %d\n255\n", S, S);
    const float L[3] = {0.3f, 0.5f, -0.81f};
    for (const Shaded& s : out) {
        unsigned char px[3] = {40, 50, 70};
        if (s.alpha == 0) transparentLeft++;
        if (s.alpha > 0) {
            (s.material == 0 ? onQuad : onPyramid)++;
            float nl = s.iN[0] * L[0] + s.iN[1] * L[1] + s.iN[2] * L[2];
            nl = 0.25f + 0.75f * (nl > 0 ? nl : 0);
            for (int k = 0; k < 3; k++) { const float c = s.albedo[k] * nl * 255.0f; px[k] = (unsigned char)(c > 255 ? 255 : c); }
        } else if (s.alpha < 0) sky++;
        fwrite(px, 1, 3, f);
    }
    fclose(f);
    printf("%zu pixels on the quad, %zu on the pyramid, %zu sky; %llu continuations in %d rounds\n", onQuad, onPyramid, sky, total, rounds + 1);

    tbvh_device_free(ctx, dRays); tbvh_device_free(ctx, dOut); tbvh_device_free(ctx, dCount);
    tbvh_shading_free(shading);
    tbvh_free_scene(tlas);
    for (int k = 0; k < 2; k++) { tbvh_free_scene(blas[k]); tbvh_host_free(host[k]); }
    tbvh_host_free(tlasHost);
    tbvh_shutdown(ctx);
    // the quad covers 4 / 5 of the window in each direction, half of its squares are holes; behind the holes the pyramid or the sky; a ray crosses the quad
    // once: the loop needs two rounds and a third that finds nothing to do
    if (onQuad < n / 5 || onPyramid < n / 50 || sky < n / 10 || total < n / 5 || transparentLeft || rounds >= 7) {
        fprintf(stderr, "unexpected picture\n");
        return 2;
    }
    printf("shaded hits ok\n");
    return 0;
}
