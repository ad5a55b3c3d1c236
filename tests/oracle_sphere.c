/* oracle_sphere.c — TEST INFRASTRUCTURE ONLY: a plain-C restatement of BVH::IntersectSphere (tiny_bvh.h:3140-3200) over the Wald BVH and
 * over the three GPU layouts the library queries (kernels_sphere.hip).  Compiled at test time by tests/sphere_lib.py
 * (cc -O2 -ffp-contract=off); the products the reference's x86 build fuses (-O3 -mavx2 -mfma, read from the disassembly of the compiled
 * function: DESIGN.md par. 11) are written as explicit fmaf, everything else is one IEEE operation per C operator.
 *
 * Spheres are {x, y, z, r}; verts are 3 x {x, y, z, w} per triangle, indexed by primitive.  Answers are one byte per sphere.
 * Walks:
 *   sph_flat       the dist2 test against one box, then every listed triangle in order (the reference with its root made one leaf)
 *   sph_wald       Wald BVH nodes (32 bytes: aabbMin, leftFirst, aabbMax, triCount) + primIdx; mode 0 = the reference verbatim, mode 1 = the
 *                  library's walk (a node taken off the stack goes through the leaf check; DESIGN.md par. 11, defect 1)
 *   sph_bvhgpu     BVH_GPU nodes (64 bytes: lmin|left, lmax|right, rmin|triCount, rmax|firstTri) + primIdx
 *   sph_bvh4       the BVH4_GPU stream (16-byte blocks, triangles inline)
 *   sph_cwbvh      BVH8_CWBVH nodes (80 bytes) + triangle records {e2, e1, v0|prim}
 * Mode 0 answers 0 / 1, plus 4 if the walk took a leaf off the stack (from there on it differs from mode 1); 2 = the reference's walk does
 * not stay defined: more than 64 stack entries, a node index outside the array, or more steps than 64 x the node count (it loops). */
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct { float x, y, z; } v3;

static v3 sub(v3 a, v3 b) { v3 r = {a.x - b.x, a.y - b.y, a.z - b.z}; return r; }
static float dot_yxz(v3 p, v3 q) { return fmaf(p.z, q.z, fmaf(p.x, q.x, p.y * q.y)); }
static float dot_xyz(v3 p, v3 q) { return fmaf(p.z, q.z, fmaf(p.y, q.y, p.x * q.x)); }
static v3 ld3(const float* p) { v3 r = {p[0], p[1], p[2]}; return r; }
static uint32_t u32(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

typedef struct { v3 pos, bmin, bmax; float r, r2; } Sph;

static Sph mk(const float* s) {
    Sph o;
    o.pos = ld3(s); o.r = s[3];
    o.bmin.x = s[0] - s[3]; o.bmin.y = s[1] - s[3]; o.bmin.z = s[2] - s[3];
    o.bmax.x = s[0] + s[3]; o.bmax.y = s[1] + s[3]; o.bmax.z = s[2] + s[3];
    o.r2 = s[3] * s[3];
    return o;
}

/* BVHNode::Intersect (tiny_bvh.h:8606-8611) */
static int overlap(const Sph* s, v3 mn, v3 mx) {
    return s->bmin.x < mx.x && s->bmax.x > mn.x && s->bmin.y < mx.y && s->bmax.y > mn.y && s->bmin.z < mx.z && s->bmax.z > mn.z;
}

/* tiny_bvh.h:3150-3157 */
static int near_box(const Sph* s, v3 mn, v3 mx) {
    float dist2 = 0.f, d;
    if (s->pos.x < mn.x) { d = mn.x - s->pos.x; dist2 = fmaf(d, d, dist2); }
    if (s->pos.x > mx.x) { d = s->pos.x - mx.x; dist2 = fmaf(d, d, dist2); }
    if (s->pos.y < mn.y) { d = mn.y - s->pos.y; dist2 = fmaf(d, d, dist2); }
    if (s->pos.y > mx.y) { d = s->pos.y - mx.y; dist2 = fmaf(d, d, dist2); }
    if (s->pos.z < mn.z) { d = mn.z - s->pos.z; dist2 = fmaf(d, d, dist2); }
    if (s->pos.z > mx.z) { d = s->pos.z - mx.z; dist2 = fmaf(d, d, dist2); }
    return dist2 <= s->r2;
}

/* tiny_bvh.h:3160-3188 */
static int tri_sphere(const Sph* s, v3 a, v3 b, v3 c) {
    const v3 A = sub(a, s->pos), B = sub(b, s->pos), C = sub(c, s->pos);
    const float rr = s->r * s->r;
    const v3 u = sub(B, A), v = sub(C, A);
    v3 V;
    V.x = fmaf(u.y, v.z, -(u.z * v.y)); V.y = fmaf(u.z, v.x, -(u.x * v.z)); V.z = fmaf(u.x, v.y, -(u.y * v.x));
    const float d = dot_yxz(A, V), e = dot_yxz(V, V);
    if (d * d > rr * e) return 0;
    const float aa = dot_yxz(A, A), ab = dot_yxz(A, B), ac = dot_yxz(A, C);
    const float bb = dot_yxz(B, B), bc = dot_yxz(B, C), cc = dot_yxz(C, C);
    if ((aa > rr && ab > aa && ac > aa) || (bb > rr && ab > bb && bc > bb) || (cc > rr && ac > cc && bc > cc)) return 0;
    const v3 AB = u, BC = sub(C, B), CA = sub(A, C);
    const float d1 = ab - aa, d2 = bc - bb, d3 = ac - cc;
    const float e1 = dot_yxz(AB, AB), e2 = dot_yxz(BC, BC), e3 = dot_xyz(CA, CA);
    v3 Q1, Q2, Q3, QC, QA, QB;
    Q1.x = fmaf(-AB.x, d1, A.x * e1); Q1.y = fmaf(-AB.y, d1, A.y * e1); Q1.z = fmaf(-AB.z, d1, A.z * e1);
    Q2.x = fmaf(-BC.x, d2, B.x * e2); Q2.y = fmaf(-BC.y, d2, B.y * e2); Q2.z = fmaf(-BC.z, d2, B.z * e2);
    Q3.x = fmaf(C.x, e3, -(CA.x * d3)); Q3.y = fmaf(C.y, e3, -(CA.y * d3)); Q3.z = fmaf(C.z, e3, -(CA.z * d3));
    QC.x = fmaf(C.x, e1, -Q1.x); QC.y = fmaf(C.y, e1, -Q1.y); QC.z = fmaf(C.z, e1, -Q1.z);
    QA.x = fmaf(A.x, e2, -Q2.x); QA.y = fmaf(A.y, e2, -Q2.y); QA.z = fmaf(A.z, e2, -Q2.z);
    QB.x = fmaf(B.x, e3, -Q3.x); QB.y = fmaf(B.y, e3, -Q3.y); QB.z = fmaf(B.z, e3, -Q3.z);
    if ((dot_yxz(Q1, Q1) > rr * e1 * e1 && dot_yxz(Q1, QC) >= 0.f) || (dot_yxz(Q2, Q2) > rr * e2 * e2 && dot_yxz(Q2, QA) >= 0.f) ||
        (dot_yxz(Q3, Q3) > rr * e3 * e3 && dot_yxz(Q3, QB) >= 0.f))
        return 0;
    return 1;
}

static int prim_hit(const Sph* s, const float* verts, uint64_t nTris, uint32_t prim) {
    if (prim >= nTris) return 0;   /* (the device skips it and reports TBVH_E_FORMAT) */
    const float* v = verts + (size_t)prim * 12;
    return tri_sphere(s, ld3(v), ld3(v + 4), ld3(v + 8));
}

void sph_flat(const float* box6, const uint32_t* primIdx, uint64_t nIdx, const float* verts, uint64_t nTris, const float* spheres, uint64_t n,
              uint8_t* out) {
    const v3 mn = ld3(box6), mx = ld3(box6 + 3);
    for (uint64_t i = 0; i < n; i++) {
        const Sph s = mk(spheres + i * 4);
        int hit = 0;
        if (near_box(&s, mn, mx))
            for (uint64_t k = 0; k < nIdx && !hit; k++) hit = prim_hit(&s, verts, nTris, primIdx[k]);
        out[i] = (uint8_t)hit;
    }
}

/* ---- Wald BVH ---------------------------------------------------------------------------------------------------------------------- */
typedef struct { float mn[3]; uint32_t leftFirst; float mx[3]; uint32_t triCount; } NodeW;

static int wald_one(const NodeW* nodes, uint64_t nNodes, const uint32_t* primIdx, uint64_t nIdx, const float* verts, uint64_t nTris, const Sph* s,
                    int mode) {
    uint64_t node = 0, stack[64], steps = 0;
    uint32_t sp = 0;
    int poppedLeaf = 0;
    for (;;) {
        if (node >= nNodes || ++steps > 64 * nNodes + 64) return 2;
        const NodeW* nd = nodes + node;
        if (nd->triCount) {
            if (near_box(s, ld3(nd->mn), ld3(nd->mx)))
                for (uint32_t i = 0; i < nd->triCount; i++) {
                    if ((uint64_t)nd->leftFirst + i >= nIdx) return 2;
                    if (prim_hit(s, verts, nTris, primIdx[nd->leftFirst + i])) return 1 | poppedLeaf;
                }
            if (sp == 0) break;
            node = stack[--sp];
            if (mode == 1) continue;
            if (node >= nNodes) return 2;
            if (nodes[node].triCount) poppedLeaf = 4;   /* the reference walks it as an interior node (tiny_bvh.h:3190-3191) */
            nd = nodes + node;
        }
        const uint64_t c1 = nd->leftFirst, c2 = (uint64_t)nd->leftFirst + 1;
        if (c2 >= nNodes) return 2;
        const int h1 = overlap(s, ld3(nodes[c1].mn), ld3(nodes[c1].mx)), h2 = overlap(s, ld3(nodes[c2].mn), ld3(nodes[c2].mx));
        if (h1 && h2) { if (sp == 64) return 2; stack[sp++] = c2; node = c1; }
        else if (h1) node = c1;
        else if (h2) node = c2;
        else { if (sp == 0) break; node = stack[--sp]; }
    }
    return poppedLeaf;
}

void sph_wald(const void* nodes32, uint64_t nNodes, const uint32_t* primIdx, uint64_t nIdx, const float* verts, uint64_t nTris, const float* spheres,
              uint64_t n, int mode, uint8_t* out) {
    for (uint64_t i = 0; i < n; i++) {
        const Sph s = mk(spheres + i * 4);
        out[i] = (uint8_t)wald_one((const NodeW*)nodes32, nNodes, primIdx, nIdx, verts, nTris, &s, mode);
    }
}

/* ---- BVH_GPU ----------------------------------------------------------------------------------------------------------------------- */
typedef struct { float lmin[3]; uint32_t left; float lmax[3]; uint32_t right; float rmin[3]; uint32_t triCount; float rmax[3]; uint32_t firstTri; } NodeAL;

/* stack entries {node, the node's box failed the leaf test}; order does not change a yes / no answer */
static int bvhgpu_one(const NodeAL* nodes, const uint32_t* primIdx, const float* verts, uint64_t nTris, const Sph* s) {
    uint32_t stack[256][2], sp = 0;
    stack[sp][0] = 0; stack[sp][1] = 0; sp++;
    while (sp) {
        sp--;
        const uint32_t ni = stack[sp][0], far = stack[sp][1];
        const NodeAL* nd = nodes + ni;
        if (nd->triCount) {
            int near = !far;
            if (ni == 0) {   /* a leaf root: the box is the min / max of its triangles' vertices */
                v3 mn = {1e30f, 1e30f, 1e30f}, mx = {-1e30f, -1e30f, -1e30f};
                for (uint32_t k = 0; k < nd->triCount; k++) {
                    const uint32_t p = primIdx[nd->firstTri + k];
                    if (p >= nTris) continue;
                    for (int j = 0; j < 3; j++) {
                        const float* v = verts + (size_t)p * 12 + j * 4;
                        mn.x = fminf(mn.x, v[0]); mn.y = fminf(mn.y, v[1]); mn.z = fminf(mn.z, v[2]);
                        mx.x = fmaxf(mx.x, v[0]); mx.y = fmaxf(mx.y, v[1]); mx.z = fmaxf(mx.z, v[2]);
                    }
                }
                near = near_box(s, mn, mx);
            }
            if (near)
                for (uint32_t k = 0; k < nd->triCount; k++)
                    if (prim_hit(s, verts, nTris, primIdx[nd->firstTri + k])) return 1;
            continue;
        }
        const v3 lmn = ld3(nd->lmin), lmx = ld3(nd->lmax), rmn = ld3(nd->rmin), rmx = ld3(nd->rmax);
        if (sp + 2 > 256) return 3;
        if (overlap(s, rmn, rmx)) { stack[sp][0] = nd->right; stack[sp][1] = !near_box(s, rmn, rmx); sp++; }
        if (overlap(s, lmn, lmx)) { stack[sp][0] = nd->left; stack[sp][1] = !near_box(s, lmn, lmx); sp++; }
    }
    return 0;
}

void sph_bvhgpu(const void* nodes64, const uint32_t* primIdx, const float* verts, uint64_t nTris, const float* spheres, uint64_t n, uint8_t* out) {
    for (uint64_t i = 0; i < n; i++) {
        const Sph s = mk(spheres + i * 4);
        out[i] = (uint8_t)bvhgpu_one((const NodeAL*)nodes64, primIdx, verts, nTris, &s);
    }
}

/* the most stack entries the last sph_bvh4 / sph_cwbvh call held at once (the kernels push the same entries in the same order) */
static uint32_t g_max_stack;
uint32_t sph_last_max_stack(void) { return g_max_stack; }

/* ---- BVH4_GPU ---------------------------------------------------------------------------------------------------------------------- */
static int bvh4_one(const float* d, const float* verts, uint64_t nTris, const Sph* s) {
    uint32_t stack[1024], sp = 0;
    stack[sp++] = 0;
    while (sp) {
        const uint32_t off = stack[--sp];
        const float* b = d + (size_t)off * 4;   /* d0 = b[0..3], d1 = b[4..7], d2 = b[8..11], d3 = b[12..15] */
        const uint32_t qx0 = u32(b[3]), qx1 = u32(b[7]), qy0 = u32(b[8]), qy1 = u32(b[9]), qz0 = u32(b[10]), qz1 = u32(b[11]);
        for (int i = 0; i < 4; i++) {
            const uint32_t info = u32(b[12 + i]);
            if (info == 0) continue;
            const int sh = 8 * i;
            v3 mn, mx;
            mn.x = b[0] + (float)((qx0 >> sh) & 255u) * b[4]; mn.y = b[1] + (float)((qy0 >> sh) & 255u) * b[5]; mn.z = b[2] + (float)((qz0 >> sh) & 255u) * b[6];
            mx.x = b[0] + (float)((qx1 >> sh) & 255u) * b[4]; mx.y = b[1] + (float)((qy1 >> sh) & 255u) * b[5]; mx.z = b[2] + (float)((qz1 >> sh) & 255u) * b[6];
            if (!overlap(s, mn, mx)) continue;
            if (info & 0x80000000u) {
                const uint32_t cnt = (info >> 16) & 0x7fffu;
                if (!cnt || !near_box(s, mn, mx)) continue;
                const uint32_t first = off + (info & 0xffffu);
                for (uint32_t k = 0; k < cnt; k++)
                    if (prim_hit(s, verts, nTris, u32(d[(size_t)(first + 3 * k) * 4 + 3]))) return 1;
            } else {
                if (sp == 1024) return 3;
                stack[sp++] = info;
                if (sp > g_max_stack) g_max_stack = sp;
            }
        }
    }
    return 0;
}

void sph_bvh4(const void* blocks16, const float* verts, uint64_t nTris, const float* spheres, uint64_t n, uint8_t* out) {
    g_max_stack = 1;
    for (uint64_t i = 0; i < n; i++) {
        const Sph s = mk(spheres + i * 4);
        out[i] = (uint8_t)bvh4_one((const float*)blocks16, verts, nTris, &s);
    }
}

/* ---- BVH8_CWBVH -------------------------------------------------------------------------------------------------------------------- */
static int popc(uint32_t x) { int c = 0; while (x) { x &= x - 1; c++; } return c; }

static int cwbvh_one(const float* nodes, const float* tris, const float* verts, uint64_t nTris, const Sph* s) {
    uint32_t stack[2048], sp = 0;
    stack[sp++] = 0;
    while (sp) {
        const float* nd = nodes + (size_t)stack[--sp] * 20;   /* n0 = nd[0..3], n1 = nd[4..7], n2..n4 = nd[8..19] */
        const uint32_t ew = u32(nd[3]), imask = ew >> 24;
        const float sx = ldexpf(1.f, (int)(int8_t)(ew & 255u)), sy = ldexpf(1.f, (int)(int8_t)((ew >> 8) & 255u)), sz = ldexpf(1.f, (int)(int8_t)((ew >> 16) & 255u));
        const uint32_t childBase = u32(nd[4]), triBase = u32(nd[5]);
        for (int slot = 0; slot < 8; slot++) {
            const int half = slot >> 2, sh = 8 * (slot & 3);
            const uint32_t meta = (u32(nd[6 + half]) >> sh) & 255u;
            if (meta == 0) continue;
            /* qlox n2.x|n2.y, qloy n2.z|n2.w, qloz n3.x|n3.y, qhix n3.z|n3.w, qhiy n4.x|n4.y, qhiz n4.z|n4.w */
            const uint32_t qlx = (u32(nd[8 + half]) >> sh) & 255u, qly = (u32(nd[10 + half]) >> sh) & 255u, qlz = (u32(nd[12 + half]) >> sh) & 255u;
            const uint32_t qhx = (u32(nd[14 + half]) >> sh) & 255u, qhy = (u32(nd[16 + half]) >> sh) & 255u, qhz = (u32(nd[18 + half]) >> sh) & 255u;
            v3 mn, mx;
            mn.x = nd[0] + (float)qlx * sx; mn.y = nd[1] + (float)qly * sy; mn.z = nd[2] + (float)qlz * sz;
            mx.x = nd[0] + (float)qhx * sx; mx.y = nd[1] + (float)qhy * sy; mx.z = nd[2] + (float)qhz * sz;
            if (!overlap(s, mn, mx)) continue;
            if (imask & (1u << slot)) {
                if (sp == 2048) return 3;
                stack[sp++] = childBase + (uint32_t)popc(imask & ((1u << slot) - 1u));
                if (sp > g_max_stack) g_max_stack = sp;
            } else if (near_box(s, mn, mx)) {
                /* triBase counts float4s, the meta offset triangles (tiny_bvh.h:5975-5999) */
                const uint32_t first = triBase + 3u * (meta & 31u), cnt = (uint32_t)popc((meta >> 5) & 7u);
                for (uint32_t k = 0; k < cnt; k++)
                    if (prim_hit(s, verts, nTris, u32(tris[(size_t)(first + 3u * k) * 4 + 11]))) return 1;
            }
        }
    }
    return 0;
}

void sph_cwbvh(const void* nodes16, const void* tris16, const float* verts, uint64_t nTris, const float* spheres, uint64_t n, uint8_t* out) {
    g_max_stack = 1;
    for (uint64_t i = 0; i < n; i++) {
        const Sph s = mk(spheres + i * 4);
        out[i] = (uint8_t)cwbvh_one((const float*)nodes16, (const float*)tris16, verts, nTris, &s);
    }
}
