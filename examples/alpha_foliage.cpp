// alpha_foliage.cpp — the load step of the reference's foliage demo (tiny_bvh_foliage.cpp:211-212: scene.CreateOpacityMicroMaps( leaves ) before the BVH of
// the mango tree is used) on the HIP engine, using only the C ABI: a few hundred leaf quads with a procedural leaf-shaped alpha texture,
//   tbvh_bake_set_opacity_micromaps( blas, &source, N )   the maps are baked on the device from UVs and texels and installed, no host round trip
// and shadow rays from the ground towards the sun counted with and without the maps: with them, light passes where the texture is transparent.
// The baked words are also read back once (tbvh_bake_opacity_micromaps) and compared with the CPU path (tbvh_host_bake_opacity_micromaps).
// Builds without the reference: the layout comes from the library's own host builder.
//
//   g++ -O2 -Iinclude examples/alpha_foliage.cpp -Ltinybvh_amd -ltinybvh_amd -Wl,-rpath,$PWD/tinybvh_amd -o examples/_build/alpha_foliage
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tinybvh_amd.h"

struct Vec4 { float x, y, z, w; };
struct UV { float u, v; };
struct Ray64 { float O[3]; uint32_t mask; float D[3]; uint32_t instIdx; float rD[3]; uint32_t inst; float t, u, v; uint32_t prim; };
static_assert(sizeof(Ray64) == 64, "record size of the C ABI");

static float safercp(float x) { return (x > 1e-12f || x < -1e-12f) ? 1.0f / x : (x >= 0 ? 1e30f : -1e30f); }
static uint32_t rngState = 0x9E3779B9u;
static float rnd() { rngState ^= rngState << 13; rngState ^= rngState >> 17; rngState ^= rngState << 5; return (float)(rngState >> 8) * (1.0f / 16777216.0f); }

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, tbvh_last_error()); return 1; } } while (0)

int main() {
    // a leaf: opaque inside a pointed oval, a hole near the tip, transparent outside (alpha in bits 24-31, as Texture::idata)
    const uint32_t TEX = 128, N = 16;
    std::vector<uint32_t> texels(TEX * TEX);
    for (uint32_t y = 0; y < TEX; y++)
        for (uint32_t x = 0; x < TEX; x++) {
            const float u = (x + 0.5f) / TEX - 0.5f, v = (y + 0.5f) / TEX;
            const float half = 0.42f * powf(sinf(3.14159265f * v), 0.8f);
            const bool hole = (u - 0.08f) * (u - 0.08f) + (v - 0.7f) * (v - 0.7f) < 0.004f;
            texels[y * TEX + x] = (fabsf(u) < half && !hole ? 0xFF000000u : 0u) | 0x2E8B57u;
        }
    // LEAVES quads (two triangles each, flat vertex array) scattered in a crown above the ground, UVs over the whole texture
    const int LEAVES = 400;
    std::vector<Vec4> verts; std::vector<UV> uvs;
    for (int i = 0; i < LEAVES; i++) {
        const float cx = rnd() * 8 - 4, cy = 3 + rnd() * 3, cz = rnd() * 8 - 4, a = rnd() * 6.2831853f, tilt = (rnd() - 0.5f) * 1.2f, s = 0.35f + 0.25f * rnd();
        const float ax[3] = {cosf(a) * s, sinf(tilt) * s * 0.5f, sinf(a) * s}, bx[3] = {-sinf(a) * s, sinf(tilt) * s, cosf(a) * s};
        const float c[4][2] = {{-1, -1}, {1, -1}, {1, 1}, {-1, 1}};
        Vec4 p[4];
        for (int k = 0; k < 4; k++) p[k] = Vec4{cx + c[k][0] * ax[0] + c[k][1] * bx[0], cy + c[k][0] * ax[1] + c[k][1] * bx[1], cz + c[k][0] * ax[2] + c[k][1] * bx[2], 0};
        const UV t[4] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
        const int tri[6] = {0, 1, 2, 0, 2, 3};
        for (int k : tri) { verts.push_back(p[k]); uvs.push_back(t[k]); }
    }
    const uint64_t nTris = verts.size() / 3;

    tbvh_context* ctx = nullptr;
    CHECK(tbvh_init(0, &ctx));
    tbvh_hostbvh* host = nullptr;
    CHECK(tbvh_host_build(verts.data(), nTris, TBVH_LAYOUT_CWBVH, nullptr, &host));
    tbvh_scene* blas = nullptr;
    CHECK(tbvh_upload_host(ctx, host, verts.data(), nTris, &blas));

    // shadow rays: a 128 x 128 grid of ground points under the crown, towards the sun
    const float sun[3] = {0.25f, 0.93f, 0.27f};
    std::vector<Ray64> rays(128 * 128);
    for (int i = 0; i < 128 * 128; i++) {
        Ray64& r = rays[i];
        memset(&r, 0, sizeof r);
        r.O[0] = ((i & 127) + 0.5f) / 128.0f * 10.0f - 6.0f; r.O[1] = 0.0f; r.O[2] = ((i >> 7) + 0.5f) / 128.0f * 10.0f - 6.0f;
        r.mask = 0xFFFF;
        for (int a = 0; a < 3; a++) { r.D[a] = sun[a]; r.rD[a] = safercp(sun[a]); }
        r.t = 1e30f;
    }
    std::vector<uint8_t> occ(rays.size());
    auto shadowed = [&](int* out) -> int {
        if (int rc = tbvh_occluded(blas, rays.data(), rays.size(), sizeof(Ray64), occ.data())) return rc;
        *out = 0;
        for (uint8_t o : occ) *out += o ? 1 : 0;
        return 0;
    };
    int plain = 0, withMaps = 0, cleared = 0;
    CHECK(shadowed(&plain));

    tbvh_alpha_texture tex = {texels.data(), TEX, TEX};
    tbvh_omm_source src;
    memset(&src, 0, sizeof src);
    src.uv = uvs.data(); src.n_uv = uvs.size(); src.uv_stride_bytes = sizeof(UV); src.on_device = 0;
    src.indices = nullptr; src.n_tris = nTris; src.tri_texture = nullptr; src.textures = &tex; src.n_textures = 1;
    CHECK(tbvh_bake_set_opacity_micromaps(blas, &src, N));
    CHECK(shadowed(&withMaps));
    CHECK(tbvh_set_opacity_micromaps(blas, nullptr, 0, 0, 0));
    CHECK(shadowed(&cleared));
    printf("%d of %zu shadow rays blocked by the leaf quads, %d with opacity micromaps (N = %u) baked on the device\n", plain, rays.size(), withMaps, N);

    // the same words read back, against the CPU path
    const uint64_t words = nTris * ((N * N + 31) / 32);
    std::vector<uint32_t> fromDevice(words), fromHost(words);
    void* dMaps = nullptr;
    CHECK(tbvh_device_malloc(ctx, words * 4, &dMaps));
    CHECK(tbvh_bake_opacity_micromaps(ctx, &src, N, (uint32_t*)dMaps));
    CHECK(tbvh_copy_from_device(ctx, fromDevice.data(), dMaps, words * 4));
    CHECK(tbvh_device_free(ctx, dMaps));
    CHECK(tbvh_host_bake_opacity_micromaps(&src, N, fromHost.data()));
    const bool same = memcmp(fromDevice.data(), fromHost.data(), words * 4) == 0;

    tbvh_free_scene(blas);
    tbvh_host_free(host);
    tbvh_shutdown(ctx);
    if (!same) { fprintf(stderr, "the device bake and the host bake differ\n"); return 2; }
    if (plain <= 0 || withMaps <= 0 || withMaps >= plain || cleared != plain) { fprintf(stderr, "the maps did not open the leaves (%d, %d, %d)\n", plain, withMaps, cleared); return 2; }
    printf("alpha foliage ok\n");
    return 0;
}
