// viewer_sanitize.cpp — a stand-alone program for a sanitizer run of the viewer frame's host twins: it calls tbvh_host_sky_sample / _sky_prepare and
// tbvh_host_viewer_generate / _continue / _shadow_rays / _light / _pack themselves (tinybvh_amd/csrc/viewer_host.cpp over viewer.h, compiled into this program:
// validation, the stride arithmetic, the arithmetic) on heap arrays of EXACTLY the sizes the entry points document — 64 or 128 bytes per ray, 48 per shading
// record, 12 per sky texel, 16 per colour, 4 per pixel, one byte per flag, nothing behind them —, on the awkward inputs the tests use: skies of 1 x 1, 7 x 5
// and 16 x 8 texels; directions on the poles, on p = +-pi, with atan2( 0, 0 ), with |D.y| beyond 1, with NaNs, infinities and huge and denormal components;
// frames of 1 x 1, 3 x 5 and 70 x 3 with first > 0; shading records with material indices beyond the table, "no surface" records, NaN and zero normals,
// colours beyond 1, negative and non-finite; and through every refusal.  Any read or write past an array, and any undefined operation (a float converted
// to an integer it does not fit), stops it.  The library's error helper (capi_context.hip) is the one thing supplied here.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -Iinclude \
//       -Itinybvh_amd/csrc tools/viewer_sanitize.cpp tinybvh_amd/csrc/viewer_host.cpp -o /tmp/viewer_sanitize && /tmp/viewer_sanitize
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

struct alignas(16) Quad { float x, y, z, w; };
static uint32_t g_seed = 12345u;
static float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)(g_seed >> 8) * (1.0f / 16777216.0f); }
static float fromBits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

#define OK(call) do { if (int rc_ = (call)) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, g_err); return 1; } } while (0)
#define REFUSED(call) do { if ((call) != TBVH_E_INVALID) { fprintf(stderr, "%s was not refused\n", #call); return 1; } } while (0)

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float awkward[] = {0.f, -0.f, 1.f, -1.f, 1.0000001f, -1.0000001f, 2.f, -2.f, 1e-45f, -1e-45f, 1e38f, -1e38f, nan, inf, -inf, 0.41421357f, 1e-20f};
    const int na = sizeof awkward / sizeof awkward[0];
    uint64_t sum = 0;
    // the sky: every triple of awkward components and 20000 random directions on three skies
    const uint32_t skies[3][2] = {{1, 1}, {7, 5}, {16, 8}};
    const uint64_t nd = (uint64_t)na * na * na + 20000;
    for (auto& wh : skies) {
        const uint32_t w = wh[0], h = wh[1];
        std::unique_ptr<float[]> px(new float[3 * w * h]);
        for (uint32_t i = 0; i < 3 * w * h; i++) px[i] = 4 * rnd();
        const float scale[3] = {1.f, 0.5f, 2.f};
        OK(tbvh_host_sky_prepare(px.get(), (uint64_t)w * h, scale, 1));
        OK(tbvh_host_sky_prepare(px.get(), (uint64_t)w * h, nullptr, 0));
        std::unique_ptr<Quad[]> dirs(new Quad[nd]), out(new Quad[nd]);
        uint64_t k = 0;
        for (int a = 0; a < na; a++) for (int b = 0; b < na; b++) for (int c = 0; c < na; c++) dirs[k++] = Quad{awkward[a], awkward[b], awkward[c], 0.f};
        for (; k < nd; k++) dirs[k] = Quad{2 * rnd() - 1, 2 * rnd() - 1, 2 * rnd() - 1, 0.f};
        OK(tbvh_host_sky_sample(px.get(), w, h, dirs.get(), nd, out.get()));
        for (uint64_t i = 0; i < nd; i++) {
            uint32_t idx; memcpy(&idx, &out[i].w, 4);
            if (idx >= w * h) { fprintf(stderr, "texel %u of a %u x %u sky\n", idx, w, h); return 1; }
            sum += idx;
        }
        OK(tbvh_host_sky_sample(nullptr, 0, 0, dirs.get(), nd, out.get()));
        REFUSED(tbvh_host_sky_sample(px.get(), 0, h, dirs.get(), nd, out.get()));
        REFUSED(tbvh_host_sky_sample(nullptr, w, h, dirs.get(), nd, out.get()));
        REFUSED(tbvh_host_sky_sample(px.get(), w, h, nullptr, nd, out.get()));
    }
    // the frames: generate, continue, shadow rays, light in both modes, pack, at strides 64 and 128
    const uint32_t SW = 7, SH = 5;
    std::unique_ptr<float[]> px(new float[3 * SW * SH]);
    for (uint32_t i = 0; i < 3 * SW * SH; i++) px[i] = 3 * rnd();
    const tbvh_material mats[3] = {{{1, 1, 1}, TBVH_OMM_NO_TEXTURE, TBVH_OMM_NO_TEXTURE}, {{1, 1, 1}, 0, TBVH_OMM_NO_TEXTURE}, {{1, 1, 1}, 9, TBVH_OMM_NO_TEXTURE}};
    const uint32_t sizes[3][2] = {{1, 1}, {3, 5}, {70, 3}};
    for (auto& wh : sizes) for (uint32_t stride : {64u, 128u}) {
        const uint64_t n = (uint64_t)wh[0] * wh[1], q = stride / 16;
        const tbvh_camera cam = {{0.3f, 0.2f, -6.0f}, {-2.5f, 2.5f, 0}, {2.5f, 2.5f, 0}, {-2.5f, -2.5f, 0}, wh[0], wh[1], 1, 1};
        std::unique_ptr<Quad[]> packed(new Quad[4 * n]), rays(new Quad[q * n]), out(new Quad[3 * n]), shadow(new Quad[4 * n]), rgb(new Quad[n]);
        std::unique_ptr<uint32_t[]> pixels(new uint32_t[n]);
        std::unique_ptr<uint8_t[]> went(new uint8_t[n]), occ(new uint8_t[n]);
        OK(tbvh_host_viewer_generate(&cam, packed.get(), 0, n));
        const uint64_t first = n / 3;
        std::unique_ptr<Quad[]> tail(new Quad[4 * (n - first)]);
        OK(tbvh_host_viewer_generate(&cam, tail.get(), first, n - first));
        if (memcmp(tail.get(), packed.get() + 4 * first, 64 * (n - first))) { fprintf(stderr, "first > 0 gives other rays\n"); return 1; }
        REFUSED(tbvh_host_viewer_generate(&cam, packed.get(), 1, n));
        REFUSED(tbvh_host_viewer_generate(nullptr, packed.get(), 0, n));
        for (uint64_t i = 0; i < n; i++) {
            Quad* r = rays.get() + q * i;
            for (uint64_t k = 0; k < q; k++) r[k] = k < 4 ? packed[4 * i + k] : Quad{7.5f, 7.5f, 7.5f, 7.5f};
            Quad* o = out.get() + 3 * i;
            const int k = (int)(i % 12);
            r[3].x = k == 0 ? 1e30f : k == 1 ? 10000.f : k == 2 ? nan : 1.0f + 20 * rnd();
            o[0] = Quad{k == 3 ? 7.5f : rnd(), k == 4 ? -3.f : rnd(), k == 5 ? inf : rnd(), k == 6 ? -1.f : (float)(i & 1)};
            o[1] = Quad{0, 0, 1, fromBits(k == 7 ? 0x80000001u : (uint32_t)(i % 3))};
            o[2] = Quad{k == 8 ? nan : rnd() - 0.5f, k == 9 ? 0.f : rnd() - 0.5f, rnd() - 0.5f, fromBits((i & 2) ? 0x00010101u : g_seed)};
            occ[i] = (uint8_t)(i & 1);
        }
        uint64_t count = 0;
        OK(tbvh_host_viewer_continue(mats, 3, 1, rays.get(), stride, out.get(), n, went.get(), &count));
        OK(tbvh_host_viewer_continue(mats, 3, 1, rays.get(), stride, out.get(), n, nullptr, nullptr));
        REFUSED(tbvh_host_viewer_continue(nullptr, 3, 1, rays.get(), stride, out.get(), n, went.get(), &count));
        REFUSED(tbvh_host_viewer_continue(mats, 3, 1, rays.get(), 72, out.get(), n, went.get(), &count));
        sum += count;
        for (int l = 0; l < na; l++) {
            const float L[3] = {awkward[l], awkward[(l + 5) % na], 0.5f};
            OK(tbvh_host_viewer_shadow_rays(rays.get(), stride, n, l ? L : nullptr, shadow.get()));
            for (uint32_t mode : {TBVH_VIEWER_GLTF, TBVH_VIEWER_FOLIAGE}) {
                OK(tbvh_host_viewer_light(mode, (l & 1) ? nullptr : px.get(), (l & 1) ? 0 : SW, (l & 1) ? 0 : SH, rays.get(), stride, out.get(), (l & 2) ? nullptr : occ.get(), n,
                                          l ? L : nullptr, rgb.get()));
                OK(tbvh_host_viewer_pack(rgb.get(), n, pixels.get()));
                for (uint64_t i = 0; i < n; i++) sum += pixels[i] & 255u;
            }
        }
        REFUSED(tbvh_host_viewer_light(2, px.get(), SW, SH, rays.get(), stride, out.get(), nullptr, n, nullptr, rgb.get()));
        REFUSED(tbvh_host_viewer_light(0, px.get(), SW, SH, rays.get(), 48, out.get(), nullptr, n, nullptr, rgb.get()));
        REFUSED(tbvh_host_viewer_light(0, px.get(), SW, SH, rays.get(), stride, nullptr, nullptr, n, nullptr, rgb.get()));
        REFUSED(tbvh_host_viewer_shadow_rays((const char*)rays.get() + 4, stride, n, nullptr, shadow.get()));
        REFUSED(tbvh_host_viewer_pack(nullptr, n, pixels.get()));
    }
    std::unique_ptr<Quad[]> c(new Quad[(size_t)na * na]);
    std::unique_ptr<uint32_t[]> p(new uint32_t[(size_t)na * na]);
    for (int a = 0; a < na; a++) for (int b = 0; b < na; b++) c[a * na + b] = Quad{awkward[a] * 1e30f, awkward[b], -awkward[a], 0.f};
    OK(tbvh_host_viewer_pack(c.get(), (uint64_t)na * na, p.get()));
    printf("viewer sanitize ok (%llu)\n", (unsigned long long)sum);
    return 0;
}
