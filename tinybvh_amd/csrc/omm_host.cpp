// omm_host.cpp — omm.h over whole host meshes, the validation of a tbvh_omm_source, and the entry point that offers both:
// tbvh_host_bake_opacity_micromaps.  Plain C++ that needs omm.h, the public header and the library's error helper only, so that it can also be compiled
// on its own (with a sanitizer, into a stand-alone program that supplies tbvh_capi::fail: tools/omm_sanitize.cpp).  Built -ffp-contract=off like the rest.
#include <string.h>

#include "omm.h"

namespace tbvh_capi {
int fail(int code, const char* fmt, ...);   // (capi_context.hip) sets tbvh_last_error() of the calling thread, returns code
}
using tbvh_capi::fail;

namespace tbvh {

static_assert(sizeof(OmmTex) == sizeof(tbvh_alpha_texture) && sizeof(OmmTex) == 16, "OmmTex is tbvh_alpha_texture");
static_assert(kOmmNoTexture == TBVH_OMM_NO_TEXTURE, "omm.h and the public header agree on the no-texture mark");

int omm_check_source(const tbvh_omm_source* src, uint32_t N, const char* who, bool hostArrays) {
    if (!src) return fail(TBVH_E_INVALID, "%s: null source", who);
    if (!omm_valid_n(N)) return fail(TBVH_E_INVALID, "%s: N = %u: a power of two from 1 to %u is taken", who, N, kOmmMaxN);
    if (!src->uv || (src->n_textures && !src->textures)) return fail(TBVH_E_INVALID, "%s: null uv or textures", who);
    if (src->n_tris == 0 || src->n_tris >> 32 || src->n_uv == 0 || src->n_uv >> 32)
        return fail(TBVH_E_INVALID, "%s: %llu triangles, %llu UVs", who, (unsigned long long)src->n_tris, (unsigned long long)src->n_uv);
    if (src->uv_stride_bytes < 8 || src->uv_stride_bytes % 4) return fail(TBVH_E_INVALID, "%s: a UV stride of %u bytes (at least 8, a multiple of 4)", who, src->uv_stride_bytes);
    if (((uintptr_t)src->uv | (uintptr_t)src->indices | (uintptr_t)src->tri_texture) & 3) return fail(TBVH_E_INVALID, "%s: uv, indices and tri_texture must be 4-byte aligned", who);
    if (!src->indices && src->n_uv < 3 * src->n_tris)
        return fail(TBVH_E_INVALID, "%s: %llu UVs for %llu triangles without indices (3 each)", who, (unsigned long long)src->n_uv, (unsigned long long)src->n_tris);
    if (!src->tri_texture && src->n_textures == 0) return fail(TBVH_E_INVALID, "%s: no tri_texture means texture 0, and there is no texture", who);
    for (uint32_t k = 0; k < src->n_textures; k++) {
        const tbvh_alpha_texture& t = src->textures[k];
        if (!t.texels || ((uintptr_t)t.texels & 3) || t.width == 0 || t.height == 0 || t.width >> 31 || t.height >> 31)
            return fail(TBVH_E_INVALID, "%s: texture %u: %u x %u texels at %p", who, k, t.width, t.height, (const void*)t.texels);
    }
    if (!hostArrays) return 0;
    if (src->indices)
        for (uint64_t i = 0; i < 3 * src->n_tris; i++)
            if (src->indices[i] >= src->n_uv)
                return fail(TBVH_E_INVALID, "%s: triangle %llu: index %u is not a UV (%llu UVs)", who, (unsigned long long)(i / 3), src->indices[i], (unsigned long long)src->n_uv);
    if (src->tri_texture)
        for (uint64_t i = 0; i < src->n_tris; i++)
            if (src->tri_texture[i] >= src->n_textures && src->tri_texture[i] != kOmmNoTexture)
                return fail(TBVH_E_INVALID, "%s: triangle %llu: texture index %u is not a texture (%u textures)", who, (unsigned long long)i, src->tri_texture[i], src->n_textures);
    return 0;
}

// (two builds of the loop, chosen when the library is loaded: on a CPU with FMA and SSE4.1 the four fmaf and the two floorf of a sample are instructions, as
// in the reference's build, instead of calls into libm — the same values either way)
#if defined(__x86_64__) && defined(__clang__)
__attribute__((target_clones("default", "arch=x86-64-v3")))
#endif
void omm_bake_host(const OmmSrc& s, uint32_t N, uint64_t first, uint64_t last, uint32_t* maps) {
    const uint32_t words = omm_words(N);
    for (uint64_t i = first; i < last; i++) {
        uint32_t* map = maps + i * words;
        OmmUV t;
        bool bad = false;
        const OmmTex* tex = omm_triangle(s, i, t, bad);
        if (!tex) { memset(map, 255, words * 4); continue; }
        memset(map, 0, words * 4);
        for (uint32_t y = 0; y < 4 * N; y++)
            for (uint32_t x = 0; x + y + 1 < 4 * N; x++) {   // (the reference's `if (u + v >= 1) break`, exact for these N)
                uint32_t idx;
                if (omm_sample(N, x, y, t, *tex, idx)) map[idx >> 5] |= 1u << (idx & 31);
            }
    }
}

}  // namespace tbvh

using namespace tbvh;

extern "C" {

int tbvh_host_bake_opacity_micromaps(const tbvh_omm_source* src, uint32_t N, uint32_t* maps_out) {
    if (src && src->on_device) return fail(TBVH_E_INVALID, "tbvh_host_bake_opacity_micromaps: the source is device-resident (tbvh_bake_opacity_micromaps takes those)");
    if (int r = omm_check_source(src, N, "tbvh_host_bake_opacity_micromaps", true)) return r;
    if (!maps_out) return fail(TBVH_E_INVALID, "tbvh_host_bake_opacity_micromaps: null output");
    const OmmSrc s = {(const char*)src->uv, src->uv_stride_bytes, (uint32_t)src->n_uv, src->indices, src->tri_texture, (const OmmTex*)src->textures, src->n_textures, src->n_tris};
    omm_bake_host(s, N, 0, src->n_tris, maps_out);
    return 0;
}

}  // extern "C"
