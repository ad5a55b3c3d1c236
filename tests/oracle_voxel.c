/* oracle_voxel.c — VoxelSet (tiny_bvh.h:988-1030, 3772-4158) restated in plain C, for the voxel tests.
 *
 * Compiled per test session by tests/voxel_lib.py with -O2 -ffp-contract=off, so every operation below is the one written.
 *   - Set / UpdateTopGrid (3786-3827): the brick map of a fixed objectDim = 256: grid 32^3 brick indices (0 = empty), bricks of 8^3
 *     values (brick 0 never written), top grid 8^3 occupancy bits over groups of 4^3 grid cells.
 *   - Setup3DDDA / Intersect / IsOccluded (3829-4156), operation for operation: the entry slab with the ternary min / max (445-446); the
 *     point along the ray as the reference build computes it (g++ -O3 -mavx2 -mfma contracts O + D * (t + 0.0000025f) into ONE fused
 *     multiply-add per component, 3846 / 3895 / 3911 / 4045 / 4061; the plane expressions are fused too, but their products are exact
 *     powers of two, so plain operations give the same bits); ceilf planes; sign bits of D from the float bits; (int) casts with x86
 *     semantics (cvttss2si: INT_MIN for NaN and out-of-range values); the int32 overload of tinybvh_clamp (458), also for the unsigned
 *     expressions of 3912-3914 / 4062-4064, so a negative offset clamps to 0; strict < between the axes.
 *   - rule 0: the reference verbatim.  Intersect writes the first filled voxel unconditionally (3920-3935); the TLAS walks a Wald-format
 *     BVH over BLASInstance records in the reference's order (IntersectTLAS / IsOccludedTLAS, 3306-3380, 3455-3519, SLAB_TEST_TWO_NODES
 *     3202-3220, the transforms with the build's contraction as oracle/tbvh_oracle.c: orc_xform_point / orc_xform_vec).
 *   - rule 1: the library's (DESIGN.md par. 10).  The first filled voxel of a set is its candidate; it is recorded only if it wins against
 *     the current hit (t < hit.t, or at equal t a found hit with a larger prim, then a larger instance); the walk itself is the reference's
 *     (t can step BACK: with a zero direction component and the origin on a cell plane a finer level's plane distance is 0, so a walk is
 *     never cut short by the t it has reached).  Occlusion is the reference's (IsOccluded compares already).  A TLAS under rule 1 visits
 *     every instance in index order (tlas nodes may be NULL): the result does not depend on the visit order, which is what makes it the
 *     device's oracle.
 * Rays are the library's 64-byte records (include/tinybvh_amd.h: O, mask, D, instIdx, rD, hit.inst, t, u, v, prim). */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define VX_FAR 1e30f
#define OBJ 256
#define BRICK 8
#define GRID 32
#define GROUP 4
#define TOP 8
#define GRID_WORDS (GRID * GRID * GRID)
#define BRICK_WORDS (BRICK * BRICK * BRICK)
#define TOP_WORDS (TOP * TOP * TOP / 32)

typedef struct {
    float O[3]; uint32_t mask;
    float D[3]; uint32_t instIdx;
    float rD[3]; uint32_t inst;
    float t, u, v; uint32_t prim;
} vx_ray;

typedef struct { const uint32_t* grid; const uint32_t* brick; const uint32_t* top; } vx_set;   /* one voxel set's three arrays */

static inline float vmin(float a, float b) { return a < b ? a : b; }   /* tinybvh_min (445) */
static inline float vmax(float a, float b) { return a > b ? a : b; }   /* tinybvh_max (446) */
static inline int32_t vclamp(int32_t x, int32_t a, int32_t b) { return x > a ? (x < b ? x : b) : a; }   /* 458 */
static inline int32_t cvt_x86(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int32_t)f : INT32_MIN; }   /* cvttss2si */
static inline float safercp(float x) { if (x > 1e-12f || x < -1e-12f) return 1.0f / x; return x >= 0 ? VX_FAR : -VX_FAR; }   /* 442 */
static inline float cull_bound(float t) { return t * 1.00000095367431640625f; }   /* device_common.h */

/* ---- Set / UpdateTopGrid (3786-3827) --------------------------------------------------------------------------------------------- */
/* grid: GRID_WORDS zeroed; bricks: room for cap bricks; *used = freeBrickPtr (1 on an empty set).  Returns 0, or -1 when cap is exceeded. */
int vx_set_voxels(uint32_t* grid, uint32_t* bricks, uint32_t cap, uint32_t* used, const uint32_t* xyzv, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t x = xyzv[i * 4], y = xyzv[i * 4 + 1], z = xyzv[i * 4 + 2], v = xyzv[i * 4 + 3];
        const uint32_t g = x / BRICK + (y / BRICK) * GRID + (z / BRICK) * GRID * GRID;
        uint32_t b = grid[g];
        if (!b) {
            if (*used == cap) return -1;
            b = grid[g] = (*used)++;
        }
        bricks[(uint64_t)b * BRICK_WORDS + (x & 7) + (y & 7) * BRICK + (z & 7) * BRICK * BRICK] = v;
    }
    return 0;
}

void vx_update_top_grid(const uint32_t* grid, uint32_t* top) {
    memset(top, 0, TOP_WORDS * 4);
    for (int x = 0; x < TOP; x++) for (int y = 0; y < TOP; y++) for (int z = 0; z < TOP; z++) {
        const uint32_t* base = grid + x * GROUP + y * GROUP * GRID + z * GROUP * GRID * GRID;
        int has = 0;
        for (int u = 0; u < GROUP && !has; u++) for (int v = 0; v < GROUP && !has; v++) for (int w = 0; w < GROUP && !has; w++)
            if (base[u + v * GRID + w * GRID * GRID]) has = 1;
        if (!has) continue;
        const uint32_t ti = x + y * TOP + z * TOP * TOP;
        top[ti >> 5] |= 1u << (ti & 31);
    }
}

/* ---- the DDA (3829-3853, 3870-4156) ---------------------------------------------------------------------------------------------- */
/* One walk over one voxel set.  Returns 1 at the first filled voxel (*tOut, *vOut), 0 on leaving the set.  STOP_NOT_BELOW: leave once the t
 * at the head of the top-level loop is not below hitT (occlusion: `while (t < hit.t)`, 4040). */
enum { STOP_NONE = 0, STOP_NOT_BELOW = 1 };
static int vx_walk(const vx_set* s, const vx_ray* r, float hitT, int stopMode, float* tOut, uint32_t* vOut) {
    uint32_t sb[3];
    float Ds[3], tm1[3], td1[3], td2[3], td3[3];
    int32_t step[3];
    for (int a = 0; a < 3; a++) {
        uint32_t bits; memcpy(&bits, &r->D[a], 4);
        sb[a] = bits >> 31;
        Ds[a] = (float)sb[a];
        step[a] = 1 - (int32_t)sb[a] * 2;
    }
    float t = 0;
    /* Setup3DDDA (3829-3853) */
    if (!(r->O[0] >= 0 && r->O[0] <= 1 && r->O[1] >= 0 && r->O[1] <= 1 && r->O[2] >= 0 && r->O[2] <= 1)) {
        const float tx1 = -r->O[0] * r->rD[0], tx2 = (1 - r->O[0]) * r->rD[0];
        float tmin = vmin(tx1, tx2), tmax = vmax(tx1, tx2);
        const float ty1 = -r->O[1] * r->rD[1], ty2 = (1 - r->O[1]) * r->rD[1];
        tmin = vmax(tmin, vmin(ty1, ty2));
        tmax = vmin(tmax, vmax(ty1, ty2));
        const float tz1 = -r->O[2] * r->rD[2], tz2 = (1 - r->O[2]) * r->rD[2];
        tmin = vmax(tmin, vmin(tz1, tz2));
        tmax = vmin(tmax, vmax(tz1, tz2));
        if (tmax < tmin || tmin > hitT || tmax < 0) return 0;
        t = tmin;
    }
    uint32_t P1[3];
    {
        const float s1 = t + 0.0000025f;
        for (int a = 0; a < 3; a++) {
            const float p = fmaf(r->D[a], s1, r->O[a]) * (float)TOP;
            const float plane = (ceilf(p) - Ds[a]) * (1.0f / TOP);
            P1[a] = (uint32_t)vclamp(cvt_x86(p), 0, TOP - 1);
            tm1[a] = (plane - r->O[a]) * r->rD[a];
            td1[a] = ((float)step[a] * (1.0f / TOP)) * r->rD[a];
        }
    }
    for (int a = 0; a < 3; a++) { td2[a] = td1[a] * (1.0f / GROUP); td3[a] = td2[a] * (1.0f / BRICK); }
    for (;;) {   /* 3883 / 4040 */
        if (stopMode == STOP_NOT_BELOW && !(t < hitT)) return 0;
        const uint32_t ti = P1[0] + P1[1] * TOP + P1[2] * TOP * TOP;
        if (s->top[ti >> 5] & (1u << (ti & 31))) {
            /* mid level (3891-3901) */
            uint32_t P2[3];
            float tm2[3];
            const float s2 = t + 0.0000025f;
            for (int a = 0; a < 3; a++) {
                const float p = fmaf(r->D[a], s2, r->O[a]) * (float)GRID;
                const float plane = (ceilf(p) - Ds[a]) * (1.0f / GRID);
                P2[a] = (uint32_t)vclamp(cvt_x86(p), (int32_t)(P1[a] * GROUP), (int32_t)(P1[a] * GROUP + (GROUP - 1)));
                tm2[a] = (plane - r->O[a]) * r->rD[a];
            }
            const uint32_t* gridBase = s->grid + ((P2[0] + P2[1] * GRID + P2[2] * GRID * GRID) & (28u + 28u * GRID + 28u * GRID * GRID));
            for (int a = 0; a < 3; a++) P2[a] &= GROUP - 1;
            for (;;) {
                const uint32_t bc = gridBase[P2[0] + P2[1] * GRID + P2[2] * GRID * GRID];
                if (bc) {
                    /* brick (3905-3917) */
                    const uint32_t* bd = s->brick + (uint64_t)bc * BRICK_WORDS;
                    uint32_t P3[3];
                    float tm3[3];
                    const float s3 = t + 0.0000025f;
                    for (int a = 0; a < 3; a++) {
                        const float p = fmaf(r->D[a], s3, r->O[a]) * (float)OBJ;
                        const uint32_t off = (uint32_t)cvt_x86(p) - (P2[a] + P1[a] * GROUP) * BRICK;   /* unsigned, as in the reference */
                        P3[a] = (uint32_t)vclamp((int32_t)off, 0, BRICK - 1);
                        const float plane = (ceilf(p) - Ds[a]) * (1.0f / OBJ);
                        tm3[a] = (plane - r->O[a]) * r->rD[a];
                    }
                    for (;;) {
                        const uint32_t v = bd[P3[0] + P3[1] * BRICK + P3[2] * BRICK * BRICK];
                        if (v) { *tOut = t; *vOut = v; return 1; }
                        int ax = tm3[0] < tm3[1] ? (tm3[0] < tm3[2] ? 0 : 2) : (tm3[1] < tm3[2] ? 1 : 2);
                        if ((P3[ax] += (uint32_t)step[ax]) >= BRICK) break;
                        t = tm3[ax]; tm3[ax] += td3[ax];
                    }
                }
                int ax = tm2[0] < tm2[1] ? (tm2[0] < tm2[2] ? 0 : 2) : (tm2[1] < tm2[2] ? 1 : 2);
                if ((P2[ax] += (uint32_t)step[ax]) >= GROUP) break;
                t = tm2[ax]; tm2[ax] += td2[ax];
            }
        }
        int ax = tm1[0] < tm1[1] ? (tm1[0] < tm1[2] ? 0 : 2) : (tm1[1] < tm1[2] ? 1 : 2);
        if ((P1[ax] += (uint32_t)step[ax]) >= TOP) break;
        t = tm1[ax]; tm1[ax] += td1[ax];
    }
    return 0;
}

/* hit_wins (device_common.h) for a voxel candidate: strictly closer, or at equal t a found hit with a larger prim, then a larger instance */
static inline int vx_wins(float t, uint32_t prim, uint32_t inst, int found, const vx_ray* r) {
    return t < r->t || (found && t == r->t && (prim < r->prim || (prim == r->prim && inst < r->inst)));
}

/* VoxelSet::Intersect on one ray; rule 0 writes unconditionally, rule 1 only a winning candidate.  found: a hit of this query so far. */
static int vx_intersect1(const vx_set* s, vx_ray* r, int rule, int found) {
    float t; uint32_t v;
    if (!vx_walk(s, r, r->t, STOP_NONE, &t, &v)) return 0;
    if (rule && !vx_wins(t, v, r->instIdx, found, r)) return 0;
    r->t = t; r->prim = v; r->inst = r->instIdx;   /* 3920-3935 (INST_IDX_BITS == 32): u, v untouched */
    return 1;
}
static int vx_occluded1(const vx_set* s, const vx_ray* r) {
    float t; uint32_t v;
    if (!vx_walk(s, r, r->t, STOP_NOT_BELOW, &t, &v)) return 0;
    return t < r->t;   /* 4038 */
}

void vx_intersect(const uint32_t* grid, const uint32_t* bricks, const uint32_t* top, void* rays, uint64_t n, int rule) {
    const vx_set s = { grid, bricks, top };
    for (uint64_t i = 0; i < n; i++) vx_intersect1(&s, (vx_ray*)rays + i, rule, 0);
}
void vx_occluded(const uint32_t* grid, const uint32_t* bricks, const uint32_t* top, const void* rays, uint64_t n, uint8_t* out) {
    const vx_set s = { grid, bricks, top };
    for (uint64_t i = 0; i < n; i++) out[i] = (uint8_t)vx_occluded1(&s, (const vx_ray*)rays + i);
}

/* ---- TLAS (3306-3380, 3455-3519) -------------------------------------------------------------------------------------------------- */
typedef struct { float mn[3]; uint32_t leftFirst; float mx[3]; uint32_t triCount; } vx_node;   /* BVH::BVHNode, 857-866 */
typedef struct {
    float transform[16], invTransform[16];
    float aabbMin[3]; uint32_t blasIdx; float aabbMax[3]; uint32_t mask; uint32_t pad[8];
} vx_instance;   /* BLASInstance, 1443-1457 */

static inline void xform_point(const float* T, const float* p, float* o) {   /* 513-522 with the reference build's contraction */
    const float rx = fmaf(T[2], p[2], fmaf(T[0], p[0], T[1] * p[1])) + T[3];
    const float ry = fmaf(T[6], p[2], fmaf(T[4], p[0], T[5] * p[1])) + T[7];
    const float rz = fmaf(T[10], p[2], fmaf(T[8], p[0], T[9] * p[1])) + T[11];
    const float w = fmaf(T[14], p[2], fmaf(T[12], p[0], T[13] * p[1])) + T[15];
    if (w == 1) { o[0] = rx; o[1] = ry; o[2] = rz; } else { const float rw = 1.f / w; o[0] = rx * rw; o[1] = ry * rw; o[2] = rz * rw; }
}
static inline void xform_vec(const float* T, const float* v, float* o) {     /* 523-528 */
    o[0] = fmaf(T[2], v[2], fmaf(T[0], v[0], T[1] * v[1]));
    o[1] = fmaf(T[6], v[2], fmaf(T[4], v[0], T[5] * v[1]));
    o[2] = fmaf(T[10], v[2], fmaf(T[8], v[0], T[9] * v[1]));
}
/* the instance's ray (3324-3333): invTransform, D not renormalised, rD = safercp(D'), instIdx = the instance index */
static void instance_ray(const vx_instance* in, uint32_t ii, const vx_ray* r, vx_ray* o) {
    *o = *r;
    xform_point(in->invTransform, r->O, o->O);
    xform_vec(in->invTransform, r->D, o->D);
    o->instIdx = ii;
    for (int a = 0; a < 3; a++) o->rD[a] = safercp(o->D[a]);
}
/* SLAB_TEST_TWO_NODES, one child (3202-3220): planes * rD - O * rD fused, tmin clamped to 0, tmax to hit.t */
static float slab(const vx_node* c, const vx_ray* r, const int pos[3], const float ro[3], float bound) {
    const float tx1 = fmaf(pos[0] ? c->mn[0] : c->mx[0], r->rD[0], -ro[0]);
    const float ty1 = fmaf(pos[1] ? c->mn[1] : c->mx[1], r->rD[1], -ro[1]);
    const float tz1 = fmaf(pos[2] ? c->mn[2] : c->mx[2], r->rD[2], -ro[2]);
    const float tx2 = fmaf(pos[0] ? c->mx[0] : c->mn[0], r->rD[0], -ro[0]);
    const float ty2 = fmaf(pos[1] ? c->mx[1] : c->mn[1], r->rD[1], -ro[1]);
    const float tz2 = fmaf(pos[2] ? c->mx[2] : c->mn[2], r->rD[2], -ro[2]);
    const float tmin = vmax(vmax(tx1, ty1), vmax(tz1, 0.0f));
    const float tmax = vmin(vmin(tx2, ty2), vmin(tz2, bound));
    return tmax >= tmin ? tmin : VX_FAR;
}

/* any: 0 = IntersectTLAS (in place), 1 = IsOccludedTLAS (returns the flag).  rule 0: the reference over the Wald nodes; rule 1: every
 * instance in index order with the library's acceptance (nodes ignored). */
static int tlas1(const vx_node* nodes, const uint32_t* idx, const vx_instance* inst, uint64_t nInst, const vx_set* sets, vx_ray* ray, int rule, int any) {
    if (rule) {
        int found = 0;
        for (uint64_t k = 0; k < nInst; k++) {
            const uint64_t ii = rule == 2 ? nInst - 1 - k : k;   /* rule 2: rule 1 in reverse index order (the tests' order-independence check) */
            const vx_instance* in = &inst[ii];
            if (!(in->mask & ray->mask)) continue;
            vx_ray tmp;
            instance_ray(in, (uint32_t)ii, ray, &tmp);
            if (any) { if (vx_occluded1(&sets[in->blasIdx], &tmp)) return 1; continue; }
            if (vx_intersect1(&sets[in->blasIdx], &tmp, 1, found)) { found = 1; ray->t = tmp.t; ray->prim = tmp.prim; ray->inst = tmp.inst; }
        }
        return 0;
    }
    const vx_node* node = &nodes[0];
    const vx_node* stack[64];
    uint32_t sp = 0;
    const int pos[3] = { ray->D[0] >= 0, ray->D[1] >= 0, ray->D[2] >= 0 };
    const float ro[3] = { ray->O[0] * ray->rD[0], ray->O[1] * ray->rD[1], ray->O[2] * ray->rD[2] };
    for (;;) {
        if (node->triCount > 0) {
            for (uint32_t i = 0; i < node->triCount; i++) {
                const uint32_t ii = idx[node->leftFirst + i];
                const vx_instance* in = &inst[ii];
                if (!(in->mask & ray->mask)) continue;   /* 3326 */
                vx_ray tmp;
                instance_ray(in, ii, ray, &tmp);
                if (any) { if (vx_occluded1(&sets[in->blasIdx], &tmp)) return 1; continue; }
                vx_intersect1(&sets[in->blasIdx], &tmp, 0, 0);   /* 3356 */
                ray->t = tmp.t; ray->u = tmp.u; ray->v = tmp.v; ray->prim = tmp.prim; ray->inst = tmp.inst;   /* 3360: ray.hit = temp.hit */
            }
            if (sp == 0) break;
            node = stack[--sp];
            continue;
        }
        const vx_node* c1 = &nodes[node->leftFirst];
        const vx_node* c2 = &nodes[node->leftFirst + 1];
        float d1 = slab(c1, ray, pos, ro, ray->t), d2 = slab(c2, ray, pos, ro, ray->t);
        if (d1 > d2) { const float tt = d1; d1 = d2; d2 = tt; const vx_node* nn = c1; c1 = c2; c2 = nn; }
        if (d1 == VX_FAR) { if (sp == 0) break; node = stack[--sp]; }
        else { node = c1; if (d2 != VX_FAR) stack[sp++] = c2; }
    }
    return 0;
}

/* sets: per blasIdx {grid, bricks, top} as three pointer arrays */
void vx_intersect_tlas(const void* nodes32, const uint32_t* idx, const void* instances192, uint64_t nInst, const uint32_t* const* grids,
                       const uint32_t* const* bricks, const uint32_t* const* tops, uint32_t nSets, void* rays, uint64_t n, int rule) {
    vx_set sets[4096];
    for (uint32_t i = 0; i < nSets && i < 4096; i++) { sets[i].grid = grids[i]; sets[i].brick = bricks[i]; sets[i].top = tops[i]; }
    for (uint64_t k = 0; k < n; k++) tlas1((const vx_node*)nodes32, idx, (const vx_instance*)instances192, nInst, sets, (vx_ray*)rays + k, rule, 0);
}
void vx_occluded_tlas(const void* nodes32, const uint32_t* idx, const void* instances192, uint64_t nInst, const uint32_t* const* grids,
                      const uint32_t* const* bricks, const uint32_t* const* tops, uint32_t nSets, const void* rays, uint64_t n, int rule, uint8_t* out) {
    vx_set sets[4096];
    for (uint32_t i = 0; i < nSets && i < 4096; i++) { sets[i].grid = grids[i]; sets[i].brick = bricks[i]; sets[i].top = tops[i]; }
    for (uint64_t k = 0; k < n; k++) {
        vx_ray r = ((const vx_ray*)rays)[k];
        out[k] = (uint8_t)tlas1((const vx_node*)nodes32, idx, (const vx_instance*)instances192, nInst, sets, &r, rule, 1);
    }
}
