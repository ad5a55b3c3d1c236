// omm_sanitize.cpp — a stand-alone program for a sanitizer run of the host micromap bake: it calls tbvh_host_bake_opacity_micromaps itself
// (tinybvh_amd/csrc/omm_host.cpp over omm.h, compiled into this program: validation, the index checks, the bake) on heap arrays of EXACTLY the sizes the
// entry point documents — UVs, indices, texture indices, texels, and an output of n_tris * words with nothing behind it —, on the awkward inputs the tests
// use (corners on integers and on texel boundaries, a tiny negative coordinate whose fraction rounds to 1, a degenerate triangle, many repeats, a 1 x 1 and
// a 37 x 19 texture, a third of the triangles without a texture), at every N, flat and indexed and strided, and through every refusal.  Non-finite UVs are
// included: the header maps them to texel 0 instead of converting a NaN.  Any read or write past an array, and any undefined operation, stops it.  The
// library's error helper (capi_context.hip) is the one thing supplied here.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Itinybvh_amd/csrc \
//       tools/omm_sanitize.cpp tinybvh_amd/csrc/omm_host.cpp -o /tmp/omm_sanitize && /tmp/omm_sanitize
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "tinybvh_amd.h"

static char g_err[512];
namespace tbvh_capi {
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace tbvh_capi

#define EXPECT(call, want) do { const int rc_ = (call); if (rc_ != (want)) { fprintf(stderr, "%s -> %d, expected %d (%s)\n", #call, rc_, (want), g_err); return 1; } } while (0)

static uint32_t rng = 0x2545f491u;
static uint32_t next() { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; return rng; }
static float unit() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }

int main() {
    const uint32_t alphas[6] = {0, 1, 2, 3, 128, 255};
    const uint32_t dims[3][2] = {{64, 64}, {37, 19}, {1, 1}};
    std::unique_ptr<uint32_t[]> texels[3];
    tbvh_alpha_texture tex[3];
    for (int k = 0; k < 3; k++) {
        const uint32_t w = dims[k][0], h = dims[k][1];
        texels[k].reset(new uint32_t[w * h]);
        for (uint32_t i = 0; i < w * h; i++) texels[k][i] = (alphas[(i / 5 + i / w / 4) % 6] << 24) | (next() & 0xFFFFFF);
        tex[k] = tbvh_alpha_texture{texels[k].get(), w, h};
    }
    const float special[][6] = {{0, 0, 1, 0, 0, 1}, {-1, 2, 2, -1, 3, 3}, {3 / 64.f, 5 / 64.f, 17 / 64.f, 5 / 64.f, 3 / 64.f, 40 / 64.f}, {-1e-9f, 0.5f, -1e-9f, 0.25f, -1e-9f, 0.75f},
                                {0.5f, -1e-9f, 0.25f, -1e-9f, 0.75f, -1e-9f}, {0.3f, 0.7f, 0.3f, 0.7f, 0.3f, 0.7f}, {-37.3f, -20.1f, 41.9f, 3.3f, 2.2f, 55.5f},
                                {NAN, 0.5f, 0.2f, 0.1f, 0.4f, 0.9f}, {INFINITY, -INFINITY, 0.2f, 0.1f, 0.4f, 0.9f}, {3e38f, -3e38f, 1e30f, 0.1f, 0.4f, 0.9f}};
    const uint64_t nSpecial = sizeof special / sizeof special[0];
    unsigned long long bits = 0;
    for (uint64_t n : {uint64_t(1), uint64_t(10), uint64_t(65), uint64_t(301)})
        for (uint32_t N : {1u, 2u, 4u, 8u, 16u, 32u, 64u})
            for (uint32_t stride : {8u, 20u}) {
                const uint32_t W = (N * N + 31) / 32;
                // flat: exactly (3 n - 1) * stride + 8 bytes of UVs
                const uint64_t uvBytes = (3 * n - 1) * stride + 8;
                std::unique_ptr<char[]> uv(new char[uvBytes]);
                memset(uv.get(), 0x7f, uvBytes);
                std::unique_ptr<uint32_t[]> tt(new uint32_t[n]), idx(new uint32_t[3 * n]), out(new uint32_t[n * W]), out2(new uint32_t[n * W]);
                for (uint64_t i = 0; i < n; i++) {
                    for (int k = 0; k < 3; k++) {
                        float c[2] = {unit() * 5 - 2, unit() * 5 - 2};
                        if (i < nSpecial) { c[0] = special[i][2 * k]; c[1] = special[i][2 * k + 1]; }
                        memcpy(uv.get() + (3 * i + k) * stride, c, 8);
                        idx[3 * i + k] = (uint32_t)(3 * (n - 1 - i) + k);   // the indexed form walks the same array backwards
                    }
                    tt[i] = i % 3 == 2 ? TBVH_OMM_NO_TEXTURE : (uint32_t)(i % 3 + (i / 3) % 2);   // textures 0, 1, 2
                }
                tbvh_omm_source src;
                memset(&src, 0, sizeof src);
                src.uv = uv.get(); src.n_uv = 3 * n; src.uv_stride_bytes = stride; src.n_tris = n; src.tri_texture = tt.get(); src.textures = tex; src.n_textures = 3;
                EXPECT(tbvh_host_bake_opacity_micromaps(&src, N, out.get()), 0);
                src.indices = idx.get();
                std::unique_ptr<uint32_t[]> ttr(new uint32_t[n]);
                for (uint64_t i = 0; i < n; i++) ttr[i] = tt[n - 1 - i];
                src.tri_texture = ttr.get();
                EXPECT(tbvh_host_bake_opacity_micromaps(&src, N, out2.get()), 0);
                for (uint64_t i = nSpecial; i < n; i++)   // (finite triangles only: a NaN's bits are unspecified, though the same code gives the same ones)
                    if (memcmp(out.get() + i * W, out2.get() + (n - 1 - i) * W, W * 4)) { fprintf(stderr, "flat and indexed differ at triangle %llu\n", (unsigned long long)i); return 1; }
                for (uint64_t i = 0; i < n * W; i++) bits += (unsigned)__builtin_popcount(out[i]);
                // refusals: nothing is written, nothing past the arrays is read
                out[0] = 0x12345678u;
                idx[3 * n - 1] = (uint32_t)(3 * n);
                EXPECT(tbvh_host_bake_opacity_micromaps(&src, N, out.get()), TBVH_E_INVALID);
                idx[3 * n - 1] = 0;
                ttr[n - 1] = 3;
                EXPECT(tbvh_host_bake_opacity_micromaps(&src, N, out.get()), TBVH_E_INVALID);
                ttr[n - 1] = 0;
                EXPECT(tbvh_host_bake_opacity_micromaps(&src, 3 * N, out.get()), TBVH_E_INVALID);   // (3, 6, 12, ...: no power of two)
                EXPECT(tbvh_host_bake_opacity_micromaps(&src, 0, out.get()), TBVH_E_INVALID);
                EXPECT(tbvh_host_bake_opacity_micromaps(&src, 128, out.get()), TBVH_E_INVALID);
                EXPECT(tbvh_host_bake_opacity_micromaps(nullptr, N, out.get()), TBVH_E_INVALID);
                EXPECT(tbvh_host_bake_opacity_micromaps(&src, N, nullptr), TBVH_E_INVALID);
                src.n_tris = 0;
                EXPECT(tbvh_host_bake_opacity_micromaps(&src, N, out.get()), TBVH_E_INVALID);
                src.n_tris = n; src.indices = nullptr; src.n_uv = 3 * n - 1;
                EXPECT(tbvh_host_bake_opacity_micromaps(&src, N, out.get()), TBVH_E_INVALID);
                if (out[0] != 0x12345678u) { fprintf(stderr, "a refused source wrote its output\n"); return 1; }
            }
    tbvh_alpha_texture empty = {texels[0].get(), 0, 64};
    float uv3[6] = {0, 0, 1, 0, 0, 1};
    uint32_t one[1];
    tbvh_omm_source src;
    memset(&src, 0, sizeof src);
    src.uv = uv3; src.n_uv = 3; src.uv_stride_bytes = 8; src.n_tris = 1; src.textures = &empty; src.n_textures = 1;
    EXPECT(tbvh_host_bake_opacity_micromaps(&src, 1, one), TBVH_E_INVALID);
    printf("omm host path: clean (%llu bits set)\n", bits);
    return 0;
}
