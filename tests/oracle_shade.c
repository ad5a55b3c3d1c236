/* oracle_shade.c — TEST INFRASTRUCTURE: GetShadingData (tiny_bvh_foliage.cpp:80-125) restated in plain C, independently of tinybvh_amd/csrc/shade.h,
 * with the contractions the reference's object code (g++ -O3 -mavx2 -mfma) has written out as fmaf calls.  Compile with -ffp-contract=off.
 * The one difference from the reference is the clamp of the texel index to width * height - 1 (DESIGN.md par. 16); flags[] says where it matters. */
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct { float color[3]; uint32_t color_texture, normal_texture; } Material;
typedef struct { const uint32_t* texels; uint32_t width, height; } Texture;
typedef struct {
    float u0, u1, u2; int32_t ltriIdx;
    float v0, v1, v2; uint32_t material;
    float vN0[3], Nx, vN1[3], Ny, vN2[3], Nz;
    float vertex0[3], u0_2, vertex1[3], u1_2, vertex2[3], u2_2;
    float T[3], area, B[3], invArea;
    float rest[8];
} FatTri;
typedef struct { float transform[16], invTransform[16], aabbMin[3]; uint32_t blasIdx; float aabbMax[3]; uint32_t mask, pad[8]; } Instance;
typedef struct { float O[3]; uint32_t mask; float D[3]; uint32_t instIdx; float rD[3]; uint32_t inst; float t, u, v; uint32_t prim; } Ray;

#define NO_TEXTURE 0xFFFFFFFFu
enum { FLAG_WRAPPED = 1, FLAG_REF_OUT_OF_BOUNDS = 2, FLAG_NO_SURFACE = 4, FLAG_BAD_INDEX = 8, FLAG_TU_INTEGER = 16 };

static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

static float dot3(const float* a, const float* b) { return fmaf(a[2], b[2], fmaf(a[0], b[0], a[1] * b[1])); }

static void transform_vector(const float* a, const float* m, float* r) {
    for (int k = 0; k < 3; k++) r[k] = fmaf(m[4 * k + 2], a[2], fmaf(m[4 * k], a[0], m[4 * k + 1] * a[1]));
}

static void normalize(float* a) {
    const float l = sqrtf(dot3(a, a));
    const float rl = l == 0 ? 0.0f : 1.0f / l;
    for (int k = 0; k < 3; k++) a[k] = a[k] * rl;
}

/* the texel the reference indexes, clamped into the texture; *flags gets FLAG_REF_OUT_OF_BOUNDS when its own index lies outside */
static uint32_t texel(const Texture* t, float tu, float tv, uint32_t* flags) {
    const int iu = (int)(tu * (float)t->width);
    const int iv = (int)(tv * (float)t->height);
    uint32_t idx = (uint32_t)iu + (uint32_t)iv * t->width;
    if (idx >= t->width * t->height) { *flags |= FLAG_REF_OUT_OF_BOUNDS; idx = t->width * t->height - 1; }
    return t->texels[idx];
}

static void no_surface(float* o) { memset(o, 0, 48); o[3] = -1.0f; }

/* instances: NULL = a single BLAS (slot 0, identity).  slot_no_surface: NULL or one byte per slot, non-zero for a BLAS without triangles (voxels,
 * spheres).  out: n x 12 floats; flags: n x u32 (may be NULL). */
void osh_shade(const Instance* instances, uint32_t n_inst, const FatTri* const* fat_tris, const uint64_t* n_tris, uint32_t n_slots, const uint8_t* slot_no_surface,
               const Material* materials, uint32_t n_materials, const Texture* textures, uint32_t n_textures, const void* rays, uint32_t stride, uint64_t n,
               float* out, uint32_t* flags_out) {
    for (uint64_t i = 0; i < n; i++) {
        const Ray* ray = (const Ray*)((const char*)rays + i * stride);
        float* o = out + 12 * i;
        uint32_t flags = 0;
        no_surface(o);
        if (ray->t >= 1e30f) { if (flags_out) flags_out[i] = FLAG_NO_SURFACE; continue; }
        const float* M = kIdentity;
        uint32_t slot = 0;
        int bad = 0;
        if (instances) {
            if (ray->inst >= n_inst) bad = 1;
            else { M = instances[ray->inst].transform; slot = instances[ray->inst].blasIdx; }
        }
        if (!bad && slot < n_slots && slot_no_surface && slot_no_surface[slot]) { if (flags_out) flags_out[i] = FLAG_NO_SURFACE; continue; }
        if (!bad && (slot >= n_slots || !fat_tris[slot] || ray->prim >= n_tris[slot])) bad = 1;
        if (bad) { if (flags_out) flags_out[i] = FLAG_NO_SURFACE | FLAG_BAD_INDEX; continue; }
        const FatTri* tri = &fat_tris[slot][ray->prim];
        Material mat = {{0, 0, 0}, NO_TEXTURE, NO_TEXTURE};
        if (tri->material < n_materials) mat = materials[tri->material]; else flags |= FLAG_BAD_INDEX;
        if (mat.color_texture != NO_TEXTURE && mat.color_texture >= n_textures) {
            flags |= FLAG_BAD_INDEX;
            mat.color[0] = mat.color[1] = mat.color[2] = 0; mat.color_texture = mat.normal_texture = NO_TEXTURE;
        }
        if (mat.normal_texture != NO_TEXTURE && mat.normal_texture >= n_textures) { flags |= FLAG_BAD_INDEX; mat.normal_texture = NO_TEXTURE; }
        const float u = ray->u, v = ray->v, w = 1 - u - v;
        float tu = fmaf(w, tri->u0, fmaf(u, tri->u1, v * tri->u2));
        float tv = fmaf(w, tri->v0, fmaf(u, tri->v1, v * tri->v2));
        if (tu == floorf(tu) || tv == floorf(tv)) flags |= FLAG_TU_INTEGER;
        tu -= floorf(tu); tv -= floorf(tv);
        if (tu == 1.0f || tv == 1.0f) flags |= FLAG_WRAPPED;
        uint32_t px = 0;
        o[3] = 1;
        if (mat.color_texture == NO_TEXTURE) memcpy(o, mat.color, 12);
        else {
            px = texel(&textures[mat.color_texture], tu, tv, &flags);
            o[0] = (float)(px & 255) * (1.0f / 256.0f);
            o[1] = (float)((px >> 8) & 255) * (1.0f / 256.0f);
            o[2] = (float)((px >> 16) & 255) * (1.0f / 256.0f);
            o[3] = (px >> 24) > 2 ? 1.0f : 0.0f;
        }
        float N[3] = {tri->Nx, tri->Ny, tri->Nz}, Nw[3];
        transform_vector(N, M, Nw);
        normalize(Nw);
        if (dot3(Nw, ray->D) > 0) for (int k = 0; k < 3; k++) Nw[k] = -Nw[k];
        float iN[3], iNw[3];
        for (int k = 0; k < 3; k++) iN[k] = fmaf(w, tri->vN0[k], fmaf(v, tri->vN2[k], u * tri->vN1[k]));
        if (mat.normal_texture != NO_TEXTURE) {
            const uint32_t p = texel(&textures[mat.normal_texture], tu, tv, &flags);
            const float mx = fmaf((float)(p & 255), 1.0f / 128.0f, -1.0f);
            const float my = fmaf((float)((p >> 8) & 255), 1.0f / 128.0f, -1.0f);
            const float mz = fmaf((float)((p >> 16) & 255), 1.0f / 128.0f, -1.0f);
            for (int k = 0; k < 3; k++) iN[k] = fmaf(mz, iN[k], fmaf(my, tri->B[k], mx * tri->T[k]));
        }
        transform_vector(iN, M, iNw);
        normalize(iNw);
        if (dot3(iNw, Nw) < 0) for (int k = 0; k < 3; k++) iNw[k] = -iNw[k];
        memcpy(o + 4, Nw, 12); memcpy(o + 7, &tri->material, 4);
        memcpy(o + 8, iNw, 12); memcpy(o + 11, &px, 4);
        if (flags_out) flags_out[i] = flags;
    }
}
