/* oracle_custom_double.c — a restatement, in plain C, of BVH_Double over custom geometry (spheres) as the reference's double demos trace it
 * (tiny_bvh_custom_double.cpp, tiny_bvh_anim_double.cpp), the checker of the sphere forms of kernels_double.hip.
 *
 * The callback is the one of tiny_bvh_anim_double.cpp, the form that stays right when |D| != 1:
 *   mag = sqrt(dot(D, D)), reciMag = 1 / mag, oc = O - pos, b = dot(oc, D) * reciMag, c = dot(oc, oc) - r * r, d = b * b - c; d <= 0 misses;
 *   t = -b - sqrt(d); a candidate iff t < tmax * mag && t > 0; it records hit.t = t * reciMag
 * every operation a separate IEEE double operation in that order (built with -O2 -ffp-contract=off: nothing is fused).
 *
 * The walks are those of oracle_double.c (BVH_Double::Intersect / IsOccluded / IntersectTLAS / IsOccludedTLAS, tiny_bvh.h:8158-8375) with the custom
 * branch in the leaves; the stack is unbounded.
 *   rule 0, the reference's: the callback sees the ray's CURRENT hit.t as tmax (the first accepted candidate shortens it for the next), box culls
 *     against hit.t, a triangle needs 0 < t < hit.t; u, v are whatever the last triangle hit left.
 *   rule 1, the library's (custom_sphere_dbl.h): a sphere candidate is checked against the record's INCOMING hit.t; the ray keeps the smallest
 *     recorded distance, then the smaller prim, then the smaller instance (triangles: hit_wins_dbl); box culls allow eight ulps
 *     (t * (1 + 2^-49)); a sphere that wins leaves u, v as the record had them.
 *   Occlusion, both rules: 1 iff some sphere is a candidate (or a triangle has 0 < t < hit.t).  The reference discards the callback's result
 *     (tiny_bvh.h:8278-8279); that defect is not restated.
 * ocd_brute tests every sphere: rule 1 is the minimum by the winner rule over all candidates, rule 0 the callback applied in index order.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

typedef struct { double mn[3], mx[3]; uint64_t leftFirst, triCount; } Node;
typedef struct { double O[3], D[3], rD[3]; double t, u, v; uint64_t inst, prim, instIdx, mask; } RayEx;
typedef struct { double transform[16], invTransform[16]; double aabbMin[3]; uint64_t blasIdx; double aabbMax[3]; uint64_t mask; } Inst;
typedef struct { double pos[3], r; } Sphere;
typedef struct { uint64_t kind; const Node* nodes; const uint64_t* idx; const void* prims; } Blas;   /* kind 0: spheres, 1: triangles (9 doubles each) */

#define DBL_FAR 1e300

static double dmin(double a, double b) { return a < b ? a : b; }
static double dmax(double a, double b) { return a > b ? a : b; }
static double bound_of(double t, int rule) { return rule ? t * 1.0000000000000017763568394002504646778106689453125 : t; }

static double node_dist(const Node* n, const double* O, const double* rD, double bound) {
    double tx1 = (n->mn[0] - O[0]) * rD[0], tx2 = (n->mx[0] - O[0]) * rD[0];
    double tmin = dmin(tx1, tx2), tmax = dmax(tx1, tx2);
    double ty1 = (n->mn[1] - O[1]) * rD[1], ty2 = (n->mx[1] - O[1]) * rD[1];
    tmin = dmax(tmin, dmin(ty1, ty2));
    tmax = dmin(tmax, dmax(ty1, ty2));
    double tz1 = (n->mn[2] - O[2]) * rD[2], tz2 = (n->mx[2] - O[2]) * rD[2];
    tmin = dmax(tmin, dmin(tz1, tz2));
    tmax = dmin(tmax, dmax(tz1, tz2));
    if (tmax >= tmin && tmin < bound && tmax >= 0) return tmin; else return DBL_FAR;
}

typedef struct { uint64_t* v; size_t n, cap; } Stack;
static void push(Stack* s, uint64_t x) {
    if (s->n == s->cap) { s->cap = s->cap ? 2 * s->cap : 256; s->v = (uint64_t*)realloc(s->v, s->cap * sizeof(uint64_t)); }
    s->v[s->n++] = x;
}

/* the callback: 1 with the recorded distance when sphere s is a candidate for a ray whose tmax is `tmax` */
static int sphere(const double* O, const double* D, const Sphere* s, double tmax, double* stored) {
    const double mag = sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]);
    const double reciMag = 1.0 / mag;
    const double oc[3] = {O[0] - s->pos[0], O[1] - s->pos[1], O[2] - s->pos[2]};
    const double b = (oc[0] * D[0] + oc[1] * D[1] + oc[2] * D[2]) * reciMag;
    const double c = (oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2]) - s->r * s->r;
    const double d = b * b - c;
    if (d <= 0) return 0;
    const double t = -b - sqrt(d);
    if (!(t < tmax * mag && t > 0)) return 0;
    *stored = t * reciMag;
    return 1;
}

static int tri(const double* O, const double* D, const double* v0, const double* v1, const double* v2, double* to, double* uo, double* vo) {
    const double e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const double e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const double h[3] = {D[1] * e2[2] - D[2] * e2[1], D[2] * e2[0] - D[0] * e2[2], D[0] * e2[1] - D[1] * e2[0]};
    const double a = e1[0] * h[0] + e1[1] * h[1] + e1[2] * h[2];
    if (fabs(a) < 0.0000001) return 0;
    const double f = 1 / a;
    const double s[3] = {O[0] - v0[0], O[1] - v0[1], O[2] - v0[2]};
    const double u = f * (s[0] * h[0] + s[1] * h[1] + s[2] * h[2]);
    const double q[3] = {s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]};
    const double v = f * (D[0] * q[0] + D[1] * q[1] + D[2] * q[2]);
    if (u < 0 || v < 0 || u + v > 1) return 0;
    *to = f * (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]);
    *uo = u; *vo = v;
    return 1;
}

/* what a ray carries besides its record: has it a hit (rule 1), and the record's incoming t, u, v */
typedef struct { int found; double tIn, uIn, vIn; } Walk;

/* one sphere against ray r (object space: O, D of r); 1: it is a candidate (the any-hit answer); closest hit: r's record is updated */
static int sphere_leaf(const Sphere* s, uint64_t p, uint64_t inst, RayEx* r, Walk* w, int rule, int any) {
    double st;
    if (!sphere(r->O, r->D, s, rule ? w->tIn : r->t, &st)) return 0;
    if (any) return 1;
    int take = 1;
    if (rule && w->found && !(st < r->t)) take = st == r->t && (p < r->prim || (p == r->prim && inst < r->inst));
    if (take) {
        r->t = st; r->prim = p; r->inst = inst; w->found = 1;
        if (rule) { r->u = w->uIn; r->v = w->vIn; }
    }
    return 1;
}

static int tri_leaf(const double* v, uint64_t p, uint64_t inst, RayEx* r, Walk* w, int rule, int any) {
    double t, u, vv;
    if (!tri(r->O, r->D, v + p * 9, v + p * 9 + 3, v + p * 9 + 6, &t, &u, &vv)) return 0;
    if (any) return t > 0 && t < r->t;
    int take;
    if (rule == 0) take = t > 0 && t < r->t;
    else take = t > 0 && (t < r->t || (w->found && t == r->t && (p < r->prim || (p == r->prim && inst < r->inst))));
    if (take) { r->t = t; r->u = u; r->v = vv; r->prim = p; r->inst = inst; w->found = 1; }
    return 0;
}

/* one BLAS; returns 1 as soon as an any-hit query is answered */
static int blas_walk(const Blas* b, RayEx* r, uint64_t inst, Walk* w, int rule, int any, Stack* st, size_t* deepest) {
    const size_t base = st->n;
    uint64_t node = 0;
    for (;;) {
        const Node* n = b->nodes + node;
        if (n->triCount > 0) {
            for (uint64_t i = 0; i < n->triCount; i++) {
                const uint64_t p = b->idx[n->leftFirst + i];
                const int hit = b->kind == 0 ? sphere_leaf((const Sphere*)b->prims + p, p, inst, r, w, rule, any) : tri_leaf((const double*)b->prims, p, inst, r, w, rule, any);
                if (any && hit) { st->n = base; return 1; }
            }
            if (st->n == base) break; else node = st->v[--st->n];
            continue;
        }
        uint64_t c1 = n->leftFirst, c2 = n->leftFirst + 1;
        const double bd = bound_of(r->t, rule);
        double d1 = node_dist(b->nodes + c1, r->O, r->rD, bd), d2 = node_dist(b->nodes + c2, r->O, r->rD, bd);
        if (d1 > d2) { double td = d1; d1 = d2; d2 = td; uint64_t tc = c1; c1 = c2; c2 = tc; }
        if (d1 == DBL_FAR) { if (st->n == base) break; else node = st->v[--st->n]; }
        else { node = c1; if (d2 != DBL_FAR) { push(st, c2); if (deepest && st->n > *deepest) *deepest = st->n; } }
    }
    return 0;
}

/* a sphere BLAS: closest hit (occ == NULL: rays are updated) or any hit (occ: one byte per ray); returns the deepest stack any ray needed */
uint64_t ocd_blas(const Node* nodes, const uint64_t* idx, const Sphere* sph, RayEx* rays, uint64_t n, int rule, uint8_t* occ) {
    Stack st = {0, 0, 0};
    size_t deepest = 0;
    const Blas b = {0, nodes, idx, sph};
    for (uint64_t i = 0; i < n; i++) {
        Walk w = {0, rays[i].t, rays[i].u, rays[i].v};
        if (occ) { RayEx r = rays[i]; occ[i] = (uint8_t)blas_walk(&b, &r, r.instIdx, &w, rule, 1, &st, &deepest); }
        else blas_walk(&b, rays + i, rays[i].instIdx, &w, rule, 0, &st, &deepest);
    }
    free(st.v);
    return deepest;
}

/* every sphere, no tree */
void ocd_brute(const Sphere* sph, uint64_t nSph, RayEx* rays, uint64_t n, int rule) {
    for (uint64_t i = 0; i < n; i++) {
        Walk w = {0, rays[i].t, rays[i].u, rays[i].v};
        for (uint64_t p = 0; p < nSph; p++) sphere_leaf(sph + p, p, rays[i].instIdx, rays + i, &w, rule, 0);
    }
}

static void xform_point(const double* v, const double* T, double* o) {
    double r[3] = {T[0] * v[0] + T[1] * v[1] + T[2] * v[2] + T[3], T[4] * v[0] + T[5] * v[1] + T[6] * v[2] + T[7], T[8] * v[0] + T[9] * v[1] + T[10] * v[2] + T[11]};
    const double w = T[12] * v[0] + T[13] * v[1] + T[14] * v[2] + T[15];
    if (w == 1) { o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; return; }
    const double rw = 1. / w;
    o[0] = r[0] * rw; o[1] = r[1] * rw; o[2] = r[2] * rw;
}
static void xform_vector(const double* v, const double* T, double* o) {
    o[0] = T[0] * v[0] + T[1] * v[1] + T[2] * v[2]; o[1] = T[4] * v[0] + T[5] * v[1] + T[6] * v[2]; o[2] = T[8] * v[0] + T[9] * v[1] + T[10] * v[2];
}
static double guarded_rcp(double d) { return d > 1e-24 ? (1.0 / d) : (d < -1e-24 ? (1.0 / d) : DBL_FAR); }

static int tlas_walk(const Node* tn, const uint64_t* tidx, const Inst* inst, const Blas* blas, RayEx* r, int rule, int any, size_t* deepest) {
    Stack st = {0, 0, 0};
    Walk w = {0, r->t, r->u, r->v};
    uint64_t node = 0;
    for (;;) {
        const Node* n = tn + node;
        if (n->triCount > 0) {
            for (uint64_t i = 0; i < n->triCount; i++) {
                const uint64_t ii = tidx[n->leftFirst + i];
                const Inst* in = inst + ii;
                if (!(in->mask & r->mask)) continue;
                RayEx tmp = *r;
                xform_point(r->O, in->invTransform, tmp.O);
                xform_vector(r->D, in->invTransform, tmp.D);
                for (int a = 0; a < 3; a++) tmp.rD[a] = any ? guarded_rcp(tmp.D[a]) : 1.0 / tmp.D[a];
                if (blas_walk(blas + in->blasIdx, &tmp, ii, &w, rule, any, &st, deepest)) { free(st.v); return 1; }
                if (!any) { r->t = tmp.t; r->u = tmp.u; r->v = tmp.v; r->prim = tmp.prim; r->inst = tmp.inst; }
            }
            if (st.n == 0) break; else node = st.v[--st.n];
            continue;
        }
        uint64_t c1 = n->leftFirst, c2 = n->leftFirst + 1;
        const double bd = bound_of(r->t, rule);
        double d1 = node_dist(tn + c1, r->O, r->rD, bd), d2 = node_dist(tn + c2, r->O, r->rD, bd);
        if (d1 > d2) { double td = d1; d1 = d2; d2 = td; uint64_t tc = c1; c1 = c2; c2 = tc; }
        if (d1 == DBL_FAR) { if (st.n == 0) break; else node = st.v[--st.n]; }
        else { node = c1; if (d2 != DBL_FAR) { push(&st, c2); if (deepest && st.n > *deepest) *deepest = st.n; } }
    }
    free(st.v);
    return 0;
}

/* a TLAS over sphere and triangle BLASes; occ == NULL: closest hit; returns the deepest stack (TLAS entries and the current BLAS's together) */
uint64_t ocd_tlas(const Node* tn, const uint64_t* tidx, const Inst* inst, const Blas* blas, RayEx* rays, uint64_t n, int rule, uint8_t* occ) {
    size_t deepest = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (occ) { RayEx r = rays[i]; occ[i] = (uint8_t)tlas_walk(tn, tidx, inst, blas, &r, rule, 1, &deepest); }
        else tlas_walk(tn, tidx, inst, blas, rays + i, rule, 0, &deepest);
    }
    return deepest;
}
