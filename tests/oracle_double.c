/* oracle_double.c — a restatement, in plain C, of tinybvh's double-precision traversals, the checker of the BVH_DOUBLE kernels.
 *
 *   BVH_Double::Intersect        tiny_bvh.h:8158-8217   od_intersect
 *   BVH_Double::IntersectTLAS    tiny_bvh.h:8220-8266   od_intersect_tlas
 *   BVH_Double::IsOccluded       tiny_bvh.h:8269-8315   od_occluded
 *   BVH_Double::IsOccludedTLAS   tiny_bvh.h:8318-8360   od_occluded_tlas
 *   BVH_Double::BVHNode::Intersect tiny_bvh.h:8363-8375 node_dist
 *   tinybvh_min / _max (double)  tiny_bvh.h:447-448; tinybvh_transform_point / _vector tiny_bvh.h:576-590
 *
 * The arithmetic is the reference's, operation for operation, in its order; compiled with -ffp-contract=off (tests/test_double_*.py) nothing is
 * fused.  Two departures, both deliberate:
 *   - the traversal stack is unbounded (the reference's stack[64] overflows on trees deeper than 64 levels);
 *   - IsOccludedTLAS tests the BLAS with the world ray's hit.t (the reference reads a RayEx it never initialised there, tiny_bvh.h:8322).
 * tie_rule 0 is the reference to the letter: a hit needs 0 < t < hit.t, so among equal distances the first found stays.  tie_rule 1 is the
 * library's rule (tinybvh_amd/csrc/device_common.h: hit_wins_dbl, cull_bound_dbl): at equal t a found hit is replaced by the smaller prim,
 * then the smaller instance, and box culls allow eight ulps (t * (1 + 2^-49)) beyond the closest hit.
 *
 * This file is not compiled against tiny_bvh.h.  It is pinned to the real reference by tests/test_double_edges_host.py (rule 0 against
 * BVH_Double::Intersect and IsOccluded on a TLAS of hostile instances, every byte) and by tests/test_double_host.py (rule 0 against a brute-force
 * fp64 closest hit over all triangles, t bit-identical where the minimum is unique).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

typedef struct { double mn[3], mx[3]; uint64_t leftFirst, triCount; } Node;
typedef struct { double O[3], D[3], rD[3]; double t, u, v; uint64_t inst, prim, instIdx, mask; } RayEx;
typedef struct { double transform[16], invTransform[16]; double aabbMin[3]; uint64_t blasIdx; double aabbMax[3]; uint64_t mask; } Inst;

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

/* Moller-Trumbore as BVH_Double::Intersect writes it (tiny_bvh.h:8177-8194); returns 1 with t, u, v when the triangle is hit with u, v inside */
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

/* One BLAS, closest hit: r->hit is updated; *found says whether r->t is a hit (rule 1) or still tmax */
static void blas_intersect(const Node* nodes, const uint64_t* idx, const double* verts, RayEx* r, uint64_t inst, int* found, int rule, Stack* st) {
    size_t base = st->n;
    uint64_t node = 0;
    for (;;) {
        const Node* n = nodes + node;
        if (n->triCount > 0) {
            for (uint64_t i = 0; i < n->triCount; i++) {
                const uint64_t p = idx[n->leftFirst + i];
                double t, u, v;
                if (!tri(r->O, r->D, verts + p * 9, verts + p * 9 + 3, verts + p * 9 + 6, &t, &u, &v)) continue;
                int take;
                if (rule == 0) take = t > 0 && t < r->t;
                else take = t > 0 && (t < r->t || (*found && t == r->t && (p < r->prim || (p == r->prim && inst < r->inst))));
                if (take) { r->t = t; r->u = u; r->v = v; r->prim = p; r->inst = inst; *found = 1; }
            }
            if (st->n == base) break; else node = st->v[--st->n];
            continue;
        }
        uint64_t c1 = n->leftFirst, c2 = n->leftFirst + 1;
        const double b = bound_of(r->t, rule);
        double d1 = node_dist(nodes + c1, r->O, r->rD, b), d2 = node_dist(nodes + c2, r->O, r->rD, b);
        if (d1 > d2) { double td = d1; d1 = d2; d2 = td; uint64_t tc = c1; c1 = c2; c2 = tc; }
        if (d1 == DBL_FAR) { if (st->n == base) break; else node = st->v[--st->n]; }
        else { node = c1; if (d2 != DBL_FAR) push(st, c2); }
    }
}

static int blas_occluded(const Node* nodes, const uint64_t* idx, const double* verts, const RayEx* r, int rule, Stack* st) {
    size_t base = st->n;
    uint64_t node = 0;
    for (;;) {
        const Node* n = nodes + node;
        if (n->triCount > 0) {
            for (uint64_t i = 0; i < n->triCount; i++) {
                const uint64_t p = idx[n->leftFirst + i];
                double t, u, v;
                if (tri(r->O, r->D, verts + p * 9, verts + p * 9 + 3, verts + p * 9 + 6, &t, &u, &v) && t > 0 && t < r->t) { st->n = base; return 1; }
            }
            if (st->n == base) break; else node = st->v[--st->n];
            continue;
        }
        uint64_t c1 = n->leftFirst, c2 = n->leftFirst + 1;
        const double b = bound_of(r->t, rule);
        double d1 = node_dist(nodes + c1, r->O, r->rD, b), d2 = node_dist(nodes + c2, r->O, r->rD, b);
        if (d1 > d2) { double td = d1; d1 = d2; d2 = td; uint64_t tc = c1; c1 = c2; c2 = tc; }
        if (d1 == DBL_FAR) { if (st->n == base) break; else node = st->v[--st->n]; }
        else { node = c1; if (d2 != DBL_FAR) push(st, c2); }
    }
    return 0;
}

void od_intersect(const Node* nodes, const uint64_t* idx, const double* verts, RayEx* rays, uint64_t n, int rule) {
    Stack st = {0, 0, 0};
    for (uint64_t i = 0; i < n; i++) { int found = 0; blas_intersect(nodes, idx, verts, rays + i, rays[i].instIdx, &found, rule, &st); }
    free(st.v);
}

void od_occluded(const Node* nodes, const uint64_t* idx, const double* verts, const RayEx* rays, uint64_t n, int rule, uint8_t* out) {
    Stack st = {0, 0, 0};
    for (uint64_t i = 0; i < n; i++) out[i] = (uint8_t)blas_occluded(nodes, idx, verts, rays + i, rule, &st);
    free(st.v);
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

/* TLAS: nodes / idx of the top level, the instances, and per BLAS its nodes, primIdx and vertices */
static void tlas_walk(const Node* tn, const uint64_t* tidx, const Inst* inst, const Node* const* bn, const uint64_t* const* bi, const double* const* bv,
                      RayEx* r, int rule, int any, uint8_t* occ) {
    Stack st = {0, 0, 0};
    int found = 0;
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
                const uint64_t b = in->blasIdx;
                if (any) {
                    for (int a = 0; a < 3; a++) tmp.rD[a] = guarded_rcp(tmp.D[a]);
                    if (blas_occluded(bn[b], bi[b], bv[b], &tmp, rule, &st)) { *occ = 1; free(st.v); return; }
                } else {
                    for (int a = 0; a < 3; a++) tmp.rD[a] = 1.0 / tmp.D[a];
                    blas_intersect(bn[b], bi[b], bv[b], &tmp, ii, &found, rule, &st);
                    r->t = tmp.t; r->u = tmp.u; r->v = tmp.v; r->prim = tmp.prim; r->inst = tmp.inst;
                }
            }
            if (st.n == 0) break; else node = st.v[--st.n];
            continue;
        }
        uint64_t c1 = n->leftFirst, c2 = n->leftFirst + 1;
        const double bd = bound_of(r->t, rule);
        double d1 = node_dist(tn + c1, r->O, r->rD, bd), d2 = node_dist(tn + c2, r->O, r->rD, bd);
        if (d1 > d2) { double td = d1; d1 = d2; d2 = td; uint64_t tc = c1; c1 = c2; c2 = tc; }
        if (d1 == DBL_FAR) { if (st.n == 0) break; else node = st.v[--st.n]; }
        else { node = c1; if (d2 != DBL_FAR) push(&st, c2); }
    }
    if (any) *occ = 0;
    free(st.v);
}

void od_intersect_tlas(const Node* tn, const uint64_t* tidx, const Inst* inst, const Node* const* bn, const uint64_t* const* bi, const double* const* bv,
                       RayEx* rays, uint64_t n, int rule) {
    for (uint64_t i = 0; i < n; i++) tlas_walk(tn, tidx, inst, bn, bi, bv, rays + i, rule, 0, 0);
}

void od_occluded_tlas(const Node* tn, const uint64_t* tidx, const Inst* inst, const Node* const* bn, const uint64_t* const* bi, const double* const* bv,
                      const RayEx* rays, uint64_t n, int rule, uint8_t* out) {
    for (uint64_t i = 0; i < n; i++) { RayEx r = rays[i]; tlas_walk(tn, tidx, inst, bn, bi, bv, &r, rule, 1, out + i); }
}
