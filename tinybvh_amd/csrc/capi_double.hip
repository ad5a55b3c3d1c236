// capi_double.hip — BVH_Double scenes (tiny_bvh.h:1035-1090): upload with validation, the _ex queries over RayEx records, and the host
// builders behind tbvh_host_build_double / tbvh_host_build_tlas_double.  The kernels are kernels_double.hip.
// A BVH_DOUBLE scene keeps its device memory in the fields every scene has (they go with the scene: tbvh_free_scene): a BLAS its nodes in
// `nodes` and its gathered triangle records in `tris`; a TLAS ONE allocation in `nodes` = [TLAS nodes | instance indices | instances | BLAS
// descriptors], each part 16-byte aligned.  Those buffers count 16-byte blocks: a NodeDbl is 4 of them, a TriDbl 5.  Nothing else of the fp32 machinery (copies, tuners, refit, updates) applies to it: the entry
// points of those refuse a BVH_DOUBLE scene.  Double scenes that move have calls of their own at the end of this file (the kernels are
// kernels_double_anim.hip): tbvh_rebuild_tlas_double_device / tbvh_update_tlas_double for a TLAS, tbvh_refit_double for a BLAS, and the downloads.
// A BVH_DOUBLE BLAS over custom geometry (spheres {pos, r}; custom_sphere_dbl.h) is the last section: `tris` holds its 48-byte records, dblSpheres
// marks it; the _ex queries and tbvh_upload_tlas_double take it, a TLAS with such a BLAS (tlas.blasSpheres) is traced by k_double's sphere forms.
#include "capi_internal.h"
#include "custom_sphere_dbl.h"

using namespace tbvh;
using namespace tbvh_capi;

namespace {

constexpr double kDblFarHost = 1e300;   // BVH_DBL_FAR, tiny_bvh.h:145

uint64_t align16(uint64_t b) { return (b + 15) & ~15ull; }

// a scene's `nodes` / `tris` buffers count 16-byte blocks: every fp64 record is a whole number of them
static_assert(sizeof(NodeDbl) % 16 == 0 && sizeof(TriDbl) % 16 == 0 && sizeof(InstanceDbl) % 16 == 0 && sizeof(BlasDbl) % 16 == 0, "fp64 records are multiples of 16 bytes");

// The checks of a caller's blob, before anything is allocated.  msg receives the first bad entry; returns TBVH_E_FORMAT or 0.
int validateDouble(const NodeDbl* n, uint64_t nNodes, const uint64_t* idx, uint64_t nIdx, uint64_t nPrims, const char* who, const char* primWhat) {
    if (nNodes == 0) return fail(TBVH_E_FORMAT, "%s: empty node array", who);
    if (nNodes >= (1ull << 32)) return fail(TBVH_E_FORMAT, "%s: %llu nodes: at most 2^32 - 1 (traversal stack entries are 32-bit)", who, (unsigned long long)nNodes);
    for (uint64_t i = 0; i < nNodes; i++) {
        const uint64_t lf = n[i].leftFirst, cnt = n[i].triCount;
        if (cnt) {
            if (lf > nIdx || cnt > nIdx - lf)
                return fail(TBVH_E_FORMAT, "%s: node %llu: leaf range [%llu, %llu + %llu) beyond n_idx = %llu", who, (unsigned long long)i, (unsigned long long)lf,
                            (unsigned long long)lf, (unsigned long long)cnt, (unsigned long long)nIdx);
        } else if (lf >= nNodes - 1)
            return fail(TBVH_E_FORMAT, "%s: node %llu: child index %llu out of range (leftFirst + 1 >= n_nodes = %llu)", who, (unsigned long long)i, (unsigned long long)lf,
                        (unsigned long long)nNodes);
    }
    for (uint64_t i = 0; i < nIdx; i++)
        if (idx[i] >= nPrims)
            return fail(TBVH_E_FORMAT, "%s: primIdx[%llu] = %llu >= %s = %llu", who, (unsigned long long)i, (unsigned long long)idx[i], primWhat, (unsigned long long)nPrims);
    // in-range indices keep every read in bounds; only a TREE keeps the traversal finite: from the root, no node may be reached twice
    std::vector<uint8_t> seen;
    std::vector<uint32_t> stack{0};
    try { seen.assign(nNodes, 0); } catch (const std::bad_alloc&) { return fail(TBVH_E_NOMEM, "%s: out of host memory", who); }
    seen[0] = 1;
    while (!stack.empty()) {
        const uint32_t i = stack.back(); stack.pop_back();
        if (n[i].triCount) continue;
        for (const uint32_t c : {(uint32_t)n[i].leftFirst, (uint32_t)n[i].leftFirst + 1u}) {
            if (seen[c]) return fail(TBVH_E_FORMAT, "%s: node %u is reachable along two paths (the node array is not a tree)", who, c);
            seen[c] = 1; stack.push_back(c);
        }
    }
    return 0;
}

bool isDouble(const tbvh_scene* s) { return s->layout == TBVH_LAYOUT_BVH_DOUBLE; }

// BLAS b as a TLAS's descriptor.  In a TLAS with a sphere BLAS (tagged) the low bit of the record pointer says which kind each BLAS is
// (k_double's sphere forms read it; records are 16-byte aligned); a TLAS of triangle BLASes keeps the plain pointers the triangle-only forms read.
BlasDbl blasDescDbl(const tbvh_scene* b, bool tagged) {
    const uintptr_t recs = (uintptr_t)b->tris.get() | (tagged && b->dblSpheres ? 1u : 0u);
    return BlasDbl{(const NodeDbl*)b->nodes.get(), (const TriDbl*)recs};
}

// TLAS parts inside its one allocation, laid out for what each part may hold (dblCap*: at upload what it holds; a device rebuild needs 2 n - 1 nodes)
struct TlasLayout { uint64_t oIdx, oInst, oBlas, total; };
TlasLayout tlasLayout(uint64_t capNodes, uint64_t capIdx, uint64_t capInst, uint64_t nBlas) {
    TlasLayout l;
    l.oIdx = align16(capNodes * sizeof(NodeDbl)); l.oInst = l.oIdx + align16(capIdx * 8); l.oBlas = l.oInst + capInst * sizeof(InstanceDbl);
    l.total = l.oBlas + nBlas * sizeof(BlasDbl);
    return l;
}
struct TlasParts { NodeDbl* nodes; uint64_t* idx; InstanceDbl* inst; BlasDbl* blas; };
TlasParts tlasParts(const tbvh_scene* s) {
    char* base = (char*)s->nodes.get();
    const TlasLayout l = tlasLayout(s->dblCapNodes, s->dblCapIdx, s->dblCapInst, s->tlas.nBlas);
    return TlasParts{(NodeDbl*)base, (uint64_t*)(base + l.oIdx), (InstanceDbl*)(base + l.oInst), (BlasDbl*)(base + l.oBlas)};
}

// one query launch on the context's stream (asynchronous), the ray pool and stack spill shared with launchQuery (capi_query.hip)
int launchDouble(tbvh_scene* s, RayExRec* dRays, uint64_t n, uint8_t* dOcc) {
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    if (n == 0) return 0;
    const size_t poolWords = (size_t)(kPoolParts + 1) * kPoolCounterStride;
    if (!c->poolClean) HIP_TRY(hipMemsetAsync(c->pool, 0, poolWords * 4 * 2, c->stream));
    c->poolClean = false;
    DoubleArgs q;
    q.rays = dRays; q.nRays = n; q.occluded = dOcc;
    q.spill = c->spill; q.spillStride = c->spillEntries;
    q.counter = (uint32_t*)c->pool + (size_t)c->poolCur * poolWords; q.counterNext = (uint32_t*)c->pool + (size_t)(c->poolCur ^ 1) * poolWords;
    q.poolParts = c->poolParts;
    q.nodes = (const NodeDbl*)s->nodes.get(); q.tris = (const TriDbl*)s->tris.get();
    q.tlasIdx = nullptr; q.inst = nullptr; q.blas = nullptr;
    if (s->isTlas) { const TlasParts p = tlasParts(s); q.tlasIdx = p.idx; q.inst = p.inst; q.blas = p.blas; }
    // one workgroup per 128 rays, at least four per CU, at most the persistent grid the spill area is sized for
    const uint64_t want = (n + 127) / 128, lo = (uint64_t)c->numCUs * 4u;
    const uint32_t blocks = (uint32_t)(want < lo ? lo : (want > c->blocks ? c->blocks : want));
    HIP_TRY(timedBegin(c));
    launch_double(s->isTlas ? s->tlas.blasSpheres : s->dblSpheres, dOcc != nullptr, s->isTlas, q, c->status, blocks, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    c->poolCur ^= 1; c->poolClean = true;
    return 0;
}

// host RayEx[] queries: one staged copy up, one launch, one copy back
int hostQueryEx(tbvh_scene* s, void* rays, uint64_t n, uint8_t* occ, const char* who) {
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    DevBuf<RayExRec> d;
    DevBuf<uint8_t> dOcc;
    if (d.alloc(n) != hipSuccess) return fail(TBVH_E_NOMEM, "%s: no device memory for %llu rays", who, (unsigned long long)n);
    if (occ && dOcc.alloc(n) != hipSuccess) return fail(TBVH_E_NOMEM, "%s: no device memory for %llu results", who, (unsigned long long)n);
    int r = 0;
    if (hipMemcpyAsync(d, rays, n * sizeof(RayExRec), hipMemcpyHostToDevice, c->stream) != hipSuccess) r = fail(TBVH_E_HIP, "%s: copy to the device failed", who);
    if (!r) r = launchDouble(s, d, n, dOcc);
    if (!r) {
        const hipError_t e = occ ? hipMemcpyAsync(occ, dOcc, n, hipMemcpyDeviceToHost, c->stream) : hipMemcpyAsync(rays, d, n * sizeof(RayExRec), hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) r = fail(TBVH_E_HIP, "%s: copy from the device failed", who);
    }
    if (!r) r = checkStatus(c);   // (synchronizes)
    else hipStreamSynchronize(c->stream);   // (either way nothing in flight reads the two buffers when they go)
    return r;
}

// ---- host builders --------------------------------------------------------------------------------------------------------------------
// The topology comes from the fp32 builders (build_bvh2 / build_bvh2_boxes) run on the input translated by its centre and rounded to float;
// every node box is then recomputed bottom-up in double from the double triangles / instance boxes, so the tree is exact and only its SAH
// quality depends on float.
void doubleFromTopology(const BVH2& b, const std::function<void(uint64_t prim, double* mn, double* mx)>& primBox, std::vector<NodeDbl>& out) {
    out.assign(b.nodes.size(), NodeDbl{});
    for (size_t i = 0; i < b.nodes.size(); i++) { out[i].leftFirst = b.nodes[i].leftFirst; out[i].triCount = b.nodes[i].triCount; }
    std::vector<uint32_t> order, stack{0};
    while (!stack.empty()) {   // pre-order from the root; reversed, children come before their parent
        const uint32_t i = stack.back(); stack.pop_back();
        order.push_back(i);
        if (!b.nodes[i].leaf()) { stack.push_back(b.nodes[i].leftFirst); stack.push_back(b.nodes[i].leftFirst + 1); }
    }
    for (size_t k = order.size(); k-- > 0;) {
        NodeDbl& n = out[order[k]];
        for (int a = 0; a < 3; a++) { n.mn[a] = kDblFarHost; n.mx[a] = -kDblFarHost; }
        if (n.triCount) {
            for (uint64_t j = 0; j < n.triCount; j++) {
                double mn[3], mx[3];
                primBox(b.primIdx[n.leftFirst + j], mn, mx);
                for (int a = 0; a < 3; a++) { n.mn[a] = std::min(n.mn[a], mn[a]); n.mx[a] = std::max(n.mx[a], mx[a]); }
            }
        } else {
            const NodeDbl &l = out[n.leftFirst], &r = out[n.leftFirst + 1];
            for (int a = 0; a < 3; a++) { n.mn[a] = std::min(l.mn[a], r.mn[a]); n.mx[a] = std::max(l.mx[a], r.mx[a]); }
        }
    }
}

// BLASInstanceEx::Update + InvertTransform (tiny_bvh.h:8432-8472), restated
void updateInstanceDbl(InstanceDbl& in, const double* bb) {
    const double* T = in.transform;
    double* iT = in.invTransform;
    iT[0] = T[5] * T[10] * T[15] - T[5] * T[11] * T[14] - T[9] * T[6] * T[15] + T[9] * T[7] * T[14] + T[13] * T[6] * T[11] - T[13] * T[7] * T[10];
    iT[1] = -T[1] * T[10] * T[15] + T[1] * T[11] * T[14] + T[9] * T[2] * T[15] - T[9] * T[3] * T[14] - T[13] * T[2] * T[11] + T[13] * T[3] * T[10];
    iT[2] = T[1] * T[6] * T[15] - T[1] * T[7] * T[14] - T[5] * T[2] * T[15] + T[5] * T[3] * T[14] + T[13] * T[2] * T[7] - T[13] * T[3] * T[6];
    iT[3] = -T[1] * T[6] * T[11] + T[1] * T[7] * T[10] + T[5] * T[2] * T[11] - T[5] * T[3] * T[10] - T[9] * T[2] * T[7] + T[9] * T[3] * T[6];
    iT[4] = -T[4] * T[10] * T[15] + T[4] * T[11] * T[14] + T[8] * T[6] * T[15] - T[8] * T[7] * T[14] - T[12] * T[6] * T[11] + T[12] * T[7] * T[10];
    iT[5] = T[0] * T[10] * T[15] - T[0] * T[11] * T[14] - T[8] * T[2] * T[15] + T[8] * T[3] * T[14] + T[12] * T[2] * T[11] - T[12] * T[3] * T[10];
    iT[6] = -T[0] * T[6] * T[15] + T[0] * T[7] * T[14] + T[4] * T[2] * T[15] - T[4] * T[3] * T[14] - T[12] * T[2] * T[7] + T[12] * T[3] * T[6];
    iT[7] = T[0] * T[6] * T[11] - T[0] * T[7] * T[10] - T[4] * T[2] * T[11] + T[4] * T[3] * T[10] + T[8] * T[2] * T[7] - T[8] * T[3] * T[6];
    iT[8] = T[4] * T[9] * T[15] - T[4] * T[11] * T[13] - T[8] * T[5] * T[15] + T[8] * T[7] * T[13] + T[12] * T[5] * T[11] - T[12] * T[7] * T[9];
    iT[9] = -T[0] * T[9] * T[15] + T[0] * T[11] * T[13] + T[8] * T[1] * T[15] - T[8] * T[3] * T[13] - T[12] * T[1] * T[11] + T[12] * T[3] * T[9];
    iT[10] = T[0] * T[5] * T[15] - T[0] * T[7] * T[13] - T[4] * T[1] * T[15] + T[4] * T[3] * T[13] + T[12] * T[1] * T[7] - T[12] * T[3] * T[5];
    iT[11] = -T[0] * T[5] * T[11] + T[0] * T[7] * T[9] + T[4] * T[1] * T[11] - T[4] * T[3] * T[9] - T[8] * T[1] * T[7] + T[8] * T[3] * T[5];
    iT[12] = -T[4] * T[9] * T[14] + T[4] * T[10] * T[13] + T[8] * T[5] * T[14] - T[8] * T[6] * T[13] - T[12] * T[5] * T[10] + T[12] * T[6] * T[9];
    iT[13] = T[0] * T[9] * T[14] - T[0] * T[10] * T[13] - T[8] * T[1] * T[14] + T[8] * T[2] * T[13] + T[12] * T[1] * T[10] - T[12] * T[2] * T[9];
    iT[14] = -T[0] * T[5] * T[14] + T[0] * T[6] * T[13] + T[4] * T[1] * T[14] - T[4] * T[2] * T[13] - T[12] * T[1] * T[6] + T[12] * T[2] * T[5];
    iT[15] = T[0] * T[5] * T[10] - T[0] * T[6] * T[9] - T[4] * T[1] * T[10] + T[4] * T[2] * T[9] + T[8] * T[1] * T[6] - T[8] * T[2] * T[5];
    const double det = T[0] * iT[0] + T[1] * iT[4] + T[2] * iT[8] + T[3] * iT[12];
    if (det != 0) {   // (the reference returns here and keeps the unscaled cofactors)
        const double invdet = 1. / det;
        for (int i = 0; i < 16; i++) iT[i] *= invdet;
    }
    const double far32 = (double)1e30f;   // aabbMin = bvhdbl3( BVH_FAR ): the float constant
    for (int a = 0; a < 3; a++) { in.aabbMin[a] = far32; in.aabbMax[a] = -far32; }
    for (int j = 0; j < 8; j++) {
        const double p[3] = {j & 1 ? bb[3] : bb[0], j & 2 ? bb[4] : bb[1], j & 4 ? bb[5] : bb[2]};
        double t[3] = {T[0] * p[0] + T[1] * p[1] + T[2] * p[2] + T[3], T[4] * p[0] + T[5] * p[1] + T[6] * p[2] + T[7], T[8] * p[0] + T[9] * p[1] + T[10] * p[2] + T[11]};
        const double w = T[12] * p[0] + T[13] * p[1] + T[14] * p[2] + T[15];
        if (w != 1) { const double rw = 1. / w; for (int a = 0; a < 3; a++) t[a] = t[a] * rw; }
        for (int a = 0; a < 3; a++) {
            in.aabbMin[a] = in.aabbMin[a] < t[a] ? in.aabbMin[a] : t[a];
            in.aabbMax[a] = in.aabbMax[a] > t[a] ? in.aabbMax[a] : t[a];
        }
    }
}

// every r finite and >= 0 (a NaN r would make a NaN box; a negative one an inverted box around a sphere the test still hits)
int validateSpheresDbl(const SphereDbl* sph, uint64_t n, const char* who) {
    for (uint64_t i = 0; i < n; i++)
        if (!(sph[i].r >= 0) || !(sph[i].r <= 1.79769313486231570815e+308))
            return fail(TBVH_E_FORMAT, "%s: sphere %llu: r = %g is not a finite number >= 0", who, (unsigned long long)i, sph[i].r);
    return 0;
}

// The two kinds of BLAS an upload makes: the caller's primitives (primBytes each) go up and `gather` makes one record of recBytes per index entry in the
// scene's `tris`.  spheres: the primitives are SphereDbl (dblSpheres); primWhat / gatherFailed: the messages' words.
struct BlasKindDbl {
    size_t primBytes, recBytes;
    void (*gather)(const uint64_t* primIdx, const void* prims, void* recs, uint64_t nIdx, hipStream_t s);
    bool spheres;
    const char *primWhat, *gatherFailed;
};
const BlasKindDbl kTriBlasDbl{72, sizeof(TriDbl), launch_gather_tris_dbl, false, "n_tris", "triangle gather failed"};
const BlasKindDbl kSphereBlasDbl{sizeof(SphereDbl), sizeof(SphereRecDbl), launch_gather_spheres_dbl, true, "n_spheres", "sphere gather failed"};

// A BLAS upload: the checks of the blob, before anything is allocated, then nodes, index list and primitives go up and the records are gathered.
int uploadBlasDbl(tbvh_context* c, const char* who, const BlasKindDbl& k, const void* nodes64, uint64_t nNodes, const uint64_t* primIdx, uint64_t nIdx,
                  const void* prims, uint64_t nPrims, tbvh_scene** out) {
    if (!c || !nodes64 || !primIdx || !prims || !out || !nIdx || !nPrims) return fail(TBVH_E_INVALID, "%s: null/empty argument", who);
    if (int r = validateDouble((const NodeDbl*)nodes64, nNodes, primIdx, nIdx, nPrims, who, k.primWhat)) return r;
    if (k.spheres)
        if (int r = validateSpheresDbl((const SphereDbl*)prims, nPrims, who)) return r;
    TBVH_ENTER(c);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_BVH_DOUBLE);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    s->dblSpheres = k.spheres;
    DevBuf<uint64_t> dIdx;
    DevBuf<double> dPrims;
    auto bail = [&](int code, const char* what) { tbvh_free_scene(s); return fail(code, "%s: %s", who, what); };
    if (s->nodes.alloc(nNodes * (sizeof(NodeDbl) / 16)) != hipSuccess || s->tris.alloc(nIdx * (k.recBytes / 16)) != hipSuccess ||
        dIdx.alloc(nIdx) != hipSuccess || dPrims.alloc(nPrims * (k.primBytes / 8)) != hipSuccess)
        return bail(TBVH_E_NOMEM, "out of device memory");
    if (hipMemcpyAsync(s->nodes, nodes64, nNodes * sizeof(NodeDbl), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(dIdx, primIdx, nIdx * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(dPrims, prims, nPrims * k.primBytes, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return bail(TBVH_E_HIP, "copy to the device failed");
    k.gather(dIdx, dPrims.get(), s->tris.get(), nIdx, c->stream);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return bail(TBVH_E_HIP, k.gatherFailed);
    s->nNodes = (uint32_t)nNodes;
    s->dblTris = nPrims; s->dblRecs = nIdx;
    *out = s;
    return 0;
}

// what the four _ex queries refuse before they look at the rays, in this order; dRays: a device ray array, or null
int checkExQuery(const tbvh_scene* s, const char* who, const void* dRays = nullptr) {
    TBVH_REFUSE_CUSTOM(s, who);
    if (!isDouble(s)) return fail(TBVH_E_INVALID, "%s: scene layout %d is not BVH_DOUBLE (RayEx queries need a BVH_Double scene)", who, s->layout);
    if (((uintptr_t)dRays) & 15) return fail(TBVH_E_INVALID, "%s: ray array must be 16-byte aligned", who);
    return 0;
}

// A double tree over n double boxes through the fp32 box builder (the recipe above): the bounds of the boxes, their centre, the boxes translated
// by it and rounded to float, build_bvh2_boxes with the caller's parameters, then every node box again in double.  h: the caller's new tbvh_hostbvh,
// which goes to *out or, on a failure, away.
int hostBuildOverBoxesDbl(tbvh_hostbvh* h, uint64_t n, const std::function<void(uint64_t i, double* mn, double* mx)>& box, const BuildParams& bp, tbvh_hostbvh** out) {
    h->layout = TBVH_LAYOUT_BVH_DOUBLE;
    try {
        double lo[3] = {kDblFarHost, kDblFarHost, kDblFarHost}, hi[3] = {-kDblFarHost, -kDblFarHost, -kDblFarHost}, mn[3], mx[3];
        for (uint64_t i = 0; i < n; i++) {
            box(i, mn, mx);
            for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], mn[a]); hi[a] = std::max(hi[a], mx[a]); }
        }
        double ctr[3];
        for (int a = 0; a < 3; a++) ctr[a] = lo[a] * 0.5 + hi[a] * 0.5;
        std::vector<float> boxes(n * 6);
        for (uint64_t i = 0; i < n; i++) {
            box(i, mn, mx);
            for (int a = 0; a < 3; a++) { boxes[i * 6 + a] = (float)(mn[a] - ctr[a]); boxes[i * 6 + 3 + a] = (float)(mx[a] - ctr[a]); }
        }
        build_bvh2_boxes(boxes.data(), (uint32_t)n, bp, h->bvh2);
        doubleFromTopology(h->bvh2, box, h->dnodes);
        h->didx.assign(h->bvh2.primIdx.begin(), h->bvh2.primIdx.end());
    } catch (const std::bad_alloc&) {
        delete h;
        return fail(TBVH_E_NOMEM, "out of host memory while building");
    }
    *out = h;
    return 0;
}

}  // namespace

extern "C" {

// ---- uploads ------------------------------------------------------------------------------------------------------------------------

int tbvh_upload_bvh_double(tbvh_context* c, const void* nodes64, uint64_t nNodes, const uint64_t* primIdx, uint64_t nIdx, const void* vertsDbl3, uint64_t nTris,
                           tbvh_scene** out) {
    return uploadBlasDbl(c, "tbvh_upload_bvh_double", kTriBlasDbl, nodes64, nNodes, primIdx, nIdx, vertsDbl3, nTris, out);
}

int tbvh_upload_tlas_double(tbvh_context* c, const void* nodes64, uint64_t nNodes, const uint64_t* idx, uint64_t nIdx, const void* instances320, uint64_t nInst,
                            tbvh_scene* const* blas, uint64_t nBlas, tbvh_scene** out) {
    if (!c || !nodes64 || !idx || !instances320 || !blas || !out || !nIdx || !nInst || !nBlas) return fail(TBVH_E_INVALID, "tbvh_upload_tlas_double: null/empty argument");
    for (uint64_t i = 0; i < nBlas; i++) {
        const tbvh_scene* b = blas[i];
        if (!b || b->ctx != c || b->isTlas || b->zombie) return fail(TBVH_E_INVALID, "tbvh_upload_tlas_double: BLAS %llu is null, freed, a TLAS, or from another context", (unsigned long long)i);
        TBVH_REFUSE_CUSTOM(b, "tbvh_upload_tlas_double");
        if (!isDouble(b)) return fail(TBVH_E_INVALID, "tbvh_upload_tlas_double: BLAS %llu has layout %d; every BLAS must be a BVH_DOUBLE scene", (unsigned long long)i, b->layout);
    }
    if (int r = validateDouble((const NodeDbl*)nodes64, nNodes, idx, nIdx, nInst, "tbvh_upload_tlas_double", "n_inst")) return r;
    const InstanceDbl* inst = (const InstanceDbl*)instances320;
    for (uint64_t i = 0; i < nInst; i++)
        if (inst[i].blasIdx >= nBlas)
            return fail(TBVH_E_FORMAT, "tbvh_upload_tlas_double: instance %llu: blasIdx %llu >= n_blas = %llu", (unsigned long long)i, (unsigned long long)inst[i].blasIdx, (unsigned long long)nBlas);
    TBVH_ENTER(c);
    bool spheres = false;
    for (uint64_t i = 0; i < nBlas; i++) spheres |= blas[i]->dblSpheres;
    std::vector<BlasDbl> descs(nBlas);
    for (uint64_t i = 0; i < nBlas; i++) descs[i] = blasDescDbl(blas[i], spheres);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_BVH_DOUBLE);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    s->isTlas = true; s->tlas.nTlasNodes = nNodes; s->tlas.nTlasIdx = nIdx; s->tlas.nInst = nInst; s->tlas.nBlas = nBlas; s->nNodes = (uint32_t)nNodes;
    s->dblCapNodes = nNodes; s->dblCapIdx = nIdx; s->dblCapInst = nInst;
    s->tlas.blasSpheres = spheres;
    const TlasLayout lay = tlasLayout(nNodes, nIdx, nInst, nBlas);
    const uint64_t oIdx = lay.oIdx, oInst = lay.oInst, oBlas = lay.oBlas, total = lay.total;
    if (s->nodes.alloc(total / 16) != hipSuccess) { tbvh_free_scene(s); return fail(TBVH_E_NOMEM, "tbvh_upload_tlas_double: out of device memory"); }
    char* base = (char*)s->nodes.get();
    if (hipMemcpyAsync(base, nodes64, nNodes * sizeof(NodeDbl), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(base + oIdx, idx, nIdx * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(base + oInst, inst, nInst * sizeof(InstanceDbl), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(base + oBlas, descs.data(), nBlas * sizeof(BlasDbl), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        tbvh_free_scene(s);
        return fail(TBVH_E_HIP, "tbvh_upload_tlas_double: copy to the device failed");
    }
    for (uint64_t i = 0; i < nBlas; i++) { s->tlas.blasList.push_back(blas[i]); blas[i]->usedBy.push_back(s); }   // (the BLASes outlive the TLAS: tbvh_free_scene)
    *out = s;
    return 0;
}

// ---- queries ----------------------------------------------------------------------------------------------------------------------

int tbvh_intersect_ex_device(tbvh_scene* s, void* dRays, uint64_t n) {
    if (!s || (!dRays && n)) return fail(TBVH_E_INVALID, "tbvh_intersect_ex_device: null argument");
    if (int r = checkExQuery(s, "tbvh_intersect_ex_device", dRays)) return r;
    return launchDouble(s, (RayExRec*)dRays, n, nullptr);
}

int tbvh_occluded_ex_device(tbvh_scene* s, const void* dRays, uint64_t n, uint8_t* dOcc) {
    if (!s || ((!dRays || !dOcc) && n)) return fail(TBVH_E_INVALID, "tbvh_occluded_ex_device: null argument");
    if (int r = checkExQuery(s, "tbvh_occluded_ex_device", dRays)) return r;
    return launchDouble(s, (RayExRec*)dRays, n, dOcc);
}

int tbvh_intersect_ex(tbvh_scene* s, void* rays, uint64_t n) {
    if (!s || (!rays && n)) return fail(TBVH_E_INVALID, "tbvh_intersect_ex: null argument");
    if (int r = checkExQuery(s, "tbvh_intersect_ex")) return r;
    if (n == 0) return 0;
    return hostQueryEx(s, rays, n, nullptr, "tbvh_intersect_ex");
}

int tbvh_occluded_ex(tbvh_scene* s, const void* rays, uint64_t n, uint8_t* occ) {
    if (!s || ((!rays || !occ) && n)) return fail(TBVH_E_INVALID, "tbvh_occluded_ex: null argument");
    if (int r = checkExQuery(s, "tbvh_occluded_ex")) return r;
    if (n == 0) return 0;
    return hostQueryEx(s, (void*)rays, n, occ, "tbvh_occluded_ex");
}

// ---- host builders ------------------------------------------------------------------------------------------------------------------

int tbvh_host_build_double(const void* vertsDbl3, uint64_t nTris, tbvh_hostbvh** out) {
    if (!vertsDbl3 || !out || nTris == 0) return fail(TBVH_E_INVALID, "tbvh_host_build_double: null/empty argument");
    if (nTris > 0x3fffffffull) return fail(TBVH_E_INVALID, "tbvh_host_build_double: too many triangles");
    const double* v = (const double*)vertsDbl3;
    tbvh_hostbvh* h = new (std::nothrow) tbvh_hostbvh;
    if (!h) return fail(TBVH_E_NOMEM, "out of host memory");
    h->layout = TBVH_LAYOUT_BVH_DOUBLE;
    try {
        double lo[3] = {kDblFarHost, kDblFarHost, kDblFarHost}, hi[3] = {-kDblFarHost, -kDblFarHost, -kDblFarHost};
        for (uint64_t i = 0; i < nTris * 3; i++)
            for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], v[i * 3 + a]); hi[a] = std::max(hi[a], v[i * 3 + a]); }
        double ctr[3];
        for (int a = 0; a < 3; a++) ctr[a] = lo[a] * 0.5 + hi[a] * 0.5;
        std::vector<Vec4> f(nTris * 3);
        for (uint64_t i = 0; i < nTris * 3; i++) f[i] = Vec4{(float)(v[i * 3] - ctr[0]), (float)(v[i * 3 + 1] - ctr[1]), (float)(v[i * 3 + 2] - ctr[2]), 0.f};
        BuildParams bp;
        bp.splitBudget = 0.f;   // every triangle in exactly one leaf
        build_bvh2(f.data(), (uint32_t)nTris, bp, h->bvh2);
        doubleFromTopology(h->bvh2, [&](uint64_t p, double* mn, double* mx) {
            for (int a = 0; a < 3; a++) {
                const double x = v[p * 9 + a], y = v[p * 9 + 3 + a], z = v[p * 9 + 6 + a];
                mn[a] = std::min(x, std::min(y, z)); mx[a] = std::max(x, std::max(y, z));
            }
        }, h->dnodes);
        h->didx.assign(h->bvh2.primIdx.begin(), h->bvh2.primIdx.end());
    } catch (const std::bad_alloc&) {
        delete h;
        return fail(TBVH_E_NOMEM, "out of host memory while building");
    }
    *out = h;
    return 0;
}

int tbvh_host_build_tlas_double(void* instances320, uint64_t nInst, const double* blasBounds6, uint64_t nBlas, tbvh_hostbvh** out) {
    if (!instances320 || !blasBounds6 || !out || nInst == 0 || nBlas == 0) return fail(TBVH_E_INVALID, "tbvh_host_build_tlas_double: null/empty argument");
    if (nInst > 0x3fffffffull) return fail(TBVH_E_INVALID, "tbvh_host_build_tlas_double: too many instances");
    InstanceDbl* inst = (InstanceDbl*)instances320;
    for (uint64_t i = 0; i < nInst; i++)
        if (inst[i].blasIdx >= nBlas) return fail(TBVH_E_INVALID, "tbvh_host_build_tlas_double: instance %llu: blasIdx %llu out of range", (unsigned long long)i, (unsigned long long)inst[i].blasIdx);
    tbvh_hostbvh* h = new (std::nothrow) tbvh_hostbvh;
    if (!h) return fail(TBVH_E_NOMEM, "out of host memory");
    for (uint64_t i = 0; i < nInst; i++) updateInstanceDbl(inst[i], blasBounds6 + 6 * inst[i].blasIdx);
    BuildParams bp; bp.maxLeafTris = 1; bp.threads = 1;   // (as tbvh_host_build_tlas)
    return hostBuildOverBoxesDbl(h, nInst, [&](uint64_t p, double* mn, double* mx) {
        for (int a = 0; a < 3; a++) { mn[a] = inst[p].aabbMin[a]; mx[a] = inst[p].aabbMax[a]; }
    }, bp, out);
}

}  // extern "C"

// ---- double scenes that move ----------------------------------------------------------------------------------------------------------

namespace {

// what every call below refuses before it looks at anything else: a null handle, an fp32 scene, a scene the caller has freed, the wrong kind
int checkDoubleScene(const tbvh_scene* s, bool wantTlas, const char* who) {
    if (!s) return fail(TBVH_E_INVALID, "%s: null scene", who);
    if (!isDouble(s)) return fail(TBVH_E_INVALID, "%s: scene layout %d is not BVH_DOUBLE", who, s->layout);
    if (s->zombie) return fail(TBVH_E_INVALID, "%s: the scene has been freed (a TLAS still holds its memory)", who);
    if (wantTlas && !s->isTlas) return fail(TBVH_E_INVALID, "%s: not a TLAS (a BVH_DOUBLE BLAS takes tbvh_refit_double / tbvh_double_download)", who);
    if (!wantTlas && s->isTlas)
        return fail(TBVH_E_INVALID, "%s: a TLAS (it takes tbvh_rebuild_tlas_double_device / tbvh_update_tlas_double / tbvh_tlas_double_download)", who);
    return 0;
}

// The TLAS in a new allocation whose parts hold capNodes / capIdx / capInst (each at least what the scene holds now): everything is carried over, the
// BLAS descriptors with it, so the scene answers as before; synchronizes, then the old allocation goes.  A failure leaves the scene as it was.
int moveTlas(tbvh_scene* s, uint64_t capNodes, uint64_t capIdx, uint64_t capInst, const char* who) {
    tbvh_context* c = s->ctx;
    const TlasLayout l = tlasLayout(capNodes, capIdx, capInst, s->tlas.nBlas);
    DevBuf<float4> fresh;
    if (fresh.alloc(l.total / 16) != hipSuccess) return fail(TBVH_E_NOMEM, "%s: out of device memory", who);
    const TlasParts o = tlasParts(s);
    char* base = (char*)fresh.get();
    if (hipMemcpyAsync(base, o.nodes, s->tlas.nTlasNodes * sizeof(NodeDbl), hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(base + l.oIdx, o.idx, s->tlas.nTlasIdx * 8, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(base + l.oInst, o.inst, s->tlas.nInst * sizeof(InstanceDbl), hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(base + l.oBlas, o.blas, s->tlas.nBlas * sizeof(BlasDbl), hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(TBVH_E_HIP, "%s: moving the TLAS failed", who);
    s->nodes = std::move(fresh);
    s->dblCapNodes = capNodes; s->dblCapIdx = capIdx; s->dblCapInst = capInst;
    return 0;
}

}  // namespace

extern "C" {

int tbvh_rebuild_tlas_double_device(tbvh_scene* s, const void* transformsDbl16, int onDevice) {
    const char* who = "tbvh_rebuild_tlas_double_device";
    if (int r = checkDoubleScene(s, true, who)) return r;
    if (transformsDbl16 && onDevice && (((uintptr_t)transformsDbl16) & 7)) return fail(TBVH_E_INVALID, "%s: device transforms must be 8-byte aligned", who);
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    const uint64_t n = s->tlas.nInst;
    if (n == 0 || n > 0x7fffffffull) return fail(TBVH_E_INVALID, "%s: %llu instances", who, (unsigned long long)n);
    // an LBVH over n leaves has 2n - 1 nodes and n index entries: the first rebuild moves an uploaded TLAS that holds fewer
    const uint64_t nNodes = 2 * n - 1;
    if (s->dblCapNodes < nNodes || s->dblCapIdx < n)
        if (int r = moveTlas(s, std::max(s->dblCapNodes, nNodes), std::max(s->dblCapIdx, n), s->dblCapInst, who)) return r;
    if (s->buildScratchFor != n) {
        s->buildScratchFor = 0;
        const size_t bytes = tlas_dbl_build_scratch_bytes((uint32_t)n, &s->sortTempBytes);
        if (s->buildScratch.alloc(bytes) != hipSuccess) return fail(TBVH_E_NOMEM, "%s: out of device memory for %zu bytes of scratch", who, bytes);
        s->buildScratchFor = n;
    }
    const double* xf = nullptr;
    if (transformsDbl16) {
        if (onDevice) xf = (const double*)transformsDbl16;
        else {
            double* stage = tlas_dbl_xform_stage(s->buildScratch, (uint32_t)n, s->sortTempBytes);
            HIP_TRY(hipMemcpyAsync(stage, transformsDbl16, n * 128, hipMemcpyHostToDevice, c->stream));
            xf = stage;
        }
    }
    const TlasParts p = tlasParts(s);
    HIP_TRY(timedBegin(c));
    HIP_TRY(launch_tlas_dbl_rebuild(p.nodes, p.idx, p.inst, p.blas, s->tlas.nBlas, xf, (uint32_t)n, s->buildScratch, s->sortTempBytes, c->stream));
    s->tlas.nTlasNodes = nNodes; s->tlas.nTlasIdx = n; s->nNodes = (uint32_t)nNodes;
    HIP_TRY(timedEnd(c));
    return 0;
}

int tbvh_update_tlas_double(tbvh_scene* s, const void* nodes64, uint64_t nNodes, const uint64_t* idx, uint64_t nIdx, const void* instances320, uint64_t nInst) {
    const char* who = "tbvh_update_tlas_double";
    if (int r = checkDoubleScene(s, true, who)) return r;
    if (!nodes64 || !idx || !instances320 || !nIdx || !nInst) return fail(TBVH_E_INVALID, "%s: null/empty argument", who);
    // the upload's checks, all of them before the scene is touched: a refused update (TBVH_E_INVALID: the scene keeps what it has) leaves the old TLAS answering
    if (validateDouble((const NodeDbl*)nodes64, nNodes, idx, nIdx, nInst, who, "n_inst")) return TBVH_E_INVALID;
    const InstanceDbl* inst = (const InstanceDbl*)instances320;
    for (uint64_t i = 0; i < nInst; i++)
        if (inst[i].blasIdx >= s->tlas.nBlas)
            return fail(TBVH_E_INVALID, "%s: instance %llu: blasIdx %llu >= n_blas = %llu", who, (unsigned long long)i, (unsigned long long)inst[i].blasIdx, (unsigned long long)s->tlas.nBlas);
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    if (nNodes > s->dblCapNodes || nIdx > s->dblCapIdx || nInst > s->dblCapInst)   // the TLAS grew
        if (int r = moveTlas(s, std::max(s->dblCapNodes, nNodes), std::max(s->dblCapIdx, nIdx), std::max(s->dblCapInst, nInst), who)) return r;
    const TlasParts p = tlasParts(s);
    if (hipMemcpyAsync(p.nodes, nodes64, nNodes * sizeof(NodeDbl), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(p.idx, idx, nIdx * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(p.inst, inst, nInst * sizeof(InstanceDbl), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)   // (the caller's arrays may go away)
        return fail(TBVH_E_HIP, "%s: copy to the device failed", who);
    s->tlas.nTlasNodes = nNodes; s->tlas.nTlasIdx = nIdx; s->tlas.nInst = nInst; s->nNodes = (uint32_t)nNodes;
    return 0;
}

int tbvh_tlas_double_download(tbvh_scene* s, void* nodes64, uint64_t capNodes, uint64_t* idx, uint64_t capIdx, void* instances320, uint64_t capInst,
                              uint64_t* nNodesOut) {
    const char* who = "tbvh_tlas_double_download";
    if (int r = checkDoubleScene(s, true, who)) return r;
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nNodesOut) *nNodesOut = s->tlas.nTlasNodes;
    if (nodes64 && capNodes < s->tlas.nTlasNodes) return fail(TBVH_E_INVALID, "%s: node buffer too small", who);
    if (idx && capIdx < s->tlas.nTlasIdx) return fail(TBVH_E_INVALID, "%s: index buffer too small", who);
    if (instances320 && capInst < s->tlas.nInst) return fail(TBVH_E_INVALID, "%s: instance buffer too small", who);
    const TlasParts p = tlasParts(s);
    if (nodes64) HIP_TRY(hipMemcpy(nodes64, p.nodes, s->tlas.nTlasNodes * sizeof(NodeDbl), hipMemcpyDeviceToHost));
    if (idx) HIP_TRY(hipMemcpy(idx, p.idx, s->tlas.nTlasIdx * 8, hipMemcpyDeviceToHost));
    if (instances320) HIP_TRY(hipMemcpy(instances320, p.inst, s->tlas.nInst * sizeof(InstanceDbl), hipMemcpyDeviceToHost));
    return 0;
}

int tbvh_double_download(tbvh_scene* s, void* nodes64, uint64_t capNodes, uint64_t* nNodesOut) {
    const char* who = "tbvh_double_download";
    if (int r = checkDoubleScene(s, false, who)) return r;
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nNodesOut) *nNodesOut = s->nNodes;
    if (nodes64 && capNodes < s->nNodes) return fail(TBVH_E_INVALID, "%s: node buffer too small", who);
    if (nodes64) HIP_TRY(hipMemcpy(nodes64, s->nodes.get(), (uint64_t)s->nNodes * sizeof(NodeDbl), hipMemcpyDeviceToHost));
    return 0;
}

int tbvh_refit_double(tbvh_scene* s, const void* vertsDbl3, uint64_t nTris, int onDevice) {
    const char* who = "tbvh_refit_double";
    if (int r = checkDoubleScene(s, false, who)) return r;
    if (s->dblSpheres) return fail(TBVH_E_INVALID, "%s: a sphere BLAS has no refit: tbvh_rebuild_custom_spheres_double_device builds it again", who);
    if (!vertsDbl3) return fail(TBVH_E_INVALID, "%s: null vertex array", who);
    if (nTris != s->dblTris) return fail(TBVH_E_INVALID, "%s: %llu triangles, the scene was uploaded with %llu", who, (unsigned long long)nTris, (unsigned long long)s->dblTris);
    if (onDevice && (((uintptr_t)vertsDbl3) & 7)) return fail(TBVH_E_INVALID, "%s: device vertices must be 8-byte aligned", who);
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    const uint32_t nNodes = s->nNodes;
    if (!s->refitScratch) {
        // first refit of the scene: parent[] | leaf list | flags, nNodes words each; the walk that fills the first two needs two frontier lists once
        DevBuf<uint32_t> fronts;
        DevBuf<void> keep;
        if (keep.alloc((size_t)nNodes * 12) != hipSuccess || fronts.alloc((size_t)nNodes * 2 + 1) != hipSuccess) return fail(TBVH_E_NOMEM, "%s: out of device memory", who);
        uint32_t* parent = (uint32_t*)keep.get();
        uint32_t nLeaves = 0;
        launch_parents_dbl((const NodeDbl*)s->nodes.get(), nNodes, parent, parent + nNodes, fronts, fronts + nNodes, fronts + 2 * (size_t)nNodes, c->stream);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&nLeaves, fronts + 2 * (size_t)nNodes, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            return fail(TBVH_E_HIP, "%s: the parent pass failed", who);
        s->refitScratch = std::move(keep);
        s->dblLeaves = nLeaves;
    }
    const double* dv = (const double*)vertsDbl3;
    if (!onDevice) {
        if (s->vertStage.reserve(nTris * 72) != hipSuccess) return fail(TBVH_E_NOMEM, "%s: out of device memory for the vertices", who);
        HIP_TRY(hipMemcpyAsync(s->vertStage, vertsDbl3, nTris * 72, hipMemcpyHostToDevice, c->stream));
        dv = (const double*)s->vertStage.get();
    }
    uint32_t* parent = (uint32_t*)s->refitScratch.get();
    HIP_TRY(timedBegin(c));
    HIP_TRY(launch_refit_dbl((NodeDbl*)s->nodes.get(), nNodes, (TriDbl*)s->tris.get(), s->dblRecs, dv, nTris, parent + nNodes, s->dblLeaves, parent, parent + 2 * (size_t)nNodes, c->stream));
    HIP_TRY(timedEnd(c));
    return 0;
}

}  // extern "C"

// ---- custom geometry: sphere BLASes (custom_sphere_dbl.h) ------------------------------------------------------------------------------------

namespace {

int checkSphereSceneDbl(const tbvh_scene* s, const char* who) {
    if (int r = checkDoubleScene(s, false, who)) return r;
    if (!s->dblSpheres) return fail(TBVH_E_INVALID, "%s: a triangle BVH_DOUBLE scene, not a sphere BLAS", who);
    return 0;
}

// A new tree over n spheres in scene s (device build).  The scene's arrays hold 2 n - 1 nodes and n records; smaller ones (a larger n, or the first rebuild
// of an uploaded scene) are replaced, and the descriptors of the TLASes over the scene re-pointed BEFORE anything is built.  n <= capacity: in place, no allocation.
int buildSphereTreeDbl(tbvh_scene* s, const char* who, const void* spheres32, uint64_t n, int onDevice) {
    tbvh_context* c = s->ctx;
    const uint64_t nNodes = 2 * n - 1, nodeBlocks = nNodes * (sizeof(NodeDbl) / 16), recBlocks = n * (sizeof(SphereRecDbl) / 16);
    if (s->buildScratchFor < n || !s->buildScratch) {
        s->buildScratchFor = 0;
        const size_t bytes = spheres_dbl_build_scratch_bytes((uint32_t)n, &s->sortTempBytes);
        if (s->buildScratch.alloc(bytes) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: out of device memory (%zu bytes of build scratch)", who, bytes); }
        s->buildScratchFor = n;
    }
    const void* dSph = spheres32;
    if (!onDevice) {
        if (s->vertStage.reserve(n * sizeof(SphereDbl)) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: out of device memory (staging %llu spheres)", who, (unsigned long long)n); }
        HIP_TRY(hipMemcpyAsync(s->vertStage, spheres32, n * sizeof(SphereDbl), hipMemcpyHostToDevice, c->stream));
        dSph = s->vertStage.get();
    }
    if (s->nodes.count() < nodeBlocks || s->tris.count() < recBlocks) {
        DevBuf<float4> nodes, recs;
        if (nodes.alloc(nodeBlocks) != hipSuccess || recs.alloc(recBlocks) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: out of device memory (%llu spheres)", who, (unsigned long long)n); }
        HIP_TRY(hipStreamSynchronize(c->stream));   // (queries in flight read the old arrays)
        DevBuf<float4> oldNodes = std::move(s->nodes), oldRecs = std::move(s->tris);
        s->nodes = std::move(nodes); s->tris = std::move(recs);
        const int r = forEachTlasOver(s, [&](tbvh_scene* t) {
            const TlasParts p = tlasParts(t);
            for (uint64_t i = 0; i < t->tlas.nBlas; i++) {
                if (t->tlas.blasList[i] != s) continue;
                const BlasDbl d = blasDescDbl(s, t->tlas.blasSpheres);
                if (hipMemcpy(p.blas + i, &d, sizeof d, hipMemcpyHostToDevice) != hipSuccess) return fail(TBVH_E_HIP, "%s: re-pointing a TLAS failed", who);
            }
            return 0;
        });
        if (r) { (void)oldNodes.release(); (void)oldRecs.release(); return r; }   // (a descriptor may still point at the old arrays: leak them rather than dangle)
    }
    HIP_TRY(timedBegin(c));
    // (a smaller n than the scratch was sized for carves smaller parts out of the same allocation)
    HIP_TRY(launch_spheres_dbl_build((NodeDbl*)s->nodes.get(), s->tris.get(), dSph, (uint32_t)n, s->buildScratch, s->sortTempBytes, c->stream));
    HIP_TRY(timedEnd(c));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (the caller's spheres may change; a launch error surfaces here)
    s->nNodes = (uint32_t)nNodes;
    s->dblTris = n; s->dblRecs = n;
    return 0;
}

}  // namespace

extern "C" {

int tbvh_upload_custom_spheres_double(tbvh_context* c, const void* nodes64, uint64_t nNodes, const uint64_t* primIdx, uint64_t nIdx, const void* spheres32,
                                      uint64_t nSpheres, tbvh_scene** out) {
    return uploadBlasDbl(c, "tbvh_upload_custom_spheres_double", kSphereBlasDbl, nodes64, nNodes, primIdx, nIdx, spheres32, nSpheres, out);
}

int tbvh_host_build_custom_spheres_double(const void* spheres32, uint64_t n, tbvh_hostbvh** out) {
    const char* who = "tbvh_host_build_custom_spheres_double";
    if (!spheres32 || !out || n == 0) return fail(TBVH_E_INVALID, "%s: null/empty argument", who);
    if (n > 0x3fffffffull) return fail(TBVH_E_INVALID, "%s: too many spheres", who);
    const SphereDbl* sph = (const SphereDbl*)spheres32;
    if (int r = validateSpheresDbl(sph, n, who)) return r;
    tbvh_hostbvh* h = new (std::nothrow) tbvh_hostbvh;
    if (!h) return fail(TBVH_E_NOMEM, "out of host memory");
    const BuildParams bp;   // (as tbvh_host_build_custom_spheres)
    return hostBuildOverBoxesDbl(h, n, [&](uint64_t p, double* mn, double* mx) { sphere_box_dbl(sph[p], mn, mx); }, bp, out);
}

int tbvh_build_device_custom_spheres_double(tbvh_context* c, const void* spheres32, uint64_t n, int onDevice, tbvh_scene** out) {
    const char* who = "tbvh_build_device_custom_spheres_double";
    if (!c || !spheres32 || !out || !n) return fail(TBVH_E_INVALID, "%s: null/empty argument", who);
    if (n > 0x7fffffffull) return fail(TBVH_E_INVALID, "%s: %llu spheres: at most 2^31 - 1", who, (unsigned long long)n);
    if (onDevice && (((uintptr_t)spheres32) & 7)) return fail(TBVH_E_INVALID, "%s: device spheres must be 8-byte aligned", who);
    TBVH_ENTER(c);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_BVH_DOUBLE);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    s->dblSpheres = true;
    if (int r = buildSphereTreeDbl(s, who, spheres32, n, onDevice)) { tbvh_free_scene(s); return r; }
    *out = s;
    return 0;
}

int tbvh_rebuild_custom_spheres_double_device(tbvh_scene* s, const void* spheres32, uint64_t n, int onDevice) {
    const char* who = "tbvh_rebuild_custom_spheres_double_device";
    if (int r = checkSphereSceneDbl(s, who)) return r;
    if (!spheres32 || !n) return fail(TBVH_E_INVALID, "%s: null/empty argument", who);
    if (n > 0x7fffffffull) return fail(TBVH_E_INVALID, "%s: %llu spheres: at most 2^31 - 1", who, (unsigned long long)n);
    if (onDevice && (((uintptr_t)spheres32) & 7)) return fail(TBVH_E_INVALID, "%s: device spheres must be 8-byte aligned", who);
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    return buildSphereTreeDbl(s, who, spheres32, n, onDevice);
}

int tbvh_custom_spheres_double_download(tbvh_scene* s, void* nodes64, uint64_t capNodes, uint64_t* primIdx, uint64_t capIdx, void* spheres32, uint64_t capSpheres,
                                        uint64_t* nNodesOut, uint64_t* nIdxOut) {
    const char* who = "tbvh_custom_spheres_double_download";
    if (int r = checkSphereSceneDbl(s, who)) return r;
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    const uint64_t nNodes = s->nNodes, nIdx = s->dblRecs;
    if (nNodesOut) *nNodesOut = nNodes;
    if (nIdxOut) *nIdxOut = nIdx;
    if (nodes64 && capNodes < nNodes) return fail(TBVH_E_INVALID, "%s: node buffer too small", who);
    if (primIdx && capIdx < nIdx) return fail(TBVH_E_INVALID, "%s: index buffer too small", who);
    if (spheres32 && capSpheres < nIdx) return fail(TBVH_E_INVALID, "%s: sphere buffer too small", who);
    if (!nodes64 && !primIdx && !spheres32) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nodes64) HIP_TRY(hipMemcpy(nodes64, s->nodes.get(), nNodes * sizeof(NodeDbl), hipMemcpyDeviceToHost));
    if (primIdx || spheres32) {   // the records {pos, r, prim, 0} come back whole and are taken apart here
        std::vector<SphereRecDbl> recs;
        try { recs.resize(nIdx); } catch (const std::bad_alloc&) { return fail(TBVH_E_NOMEM, "out of host memory"); }
        HIP_TRY(hipMemcpy(recs.data(), s->tris.get(), nIdx * sizeof(SphereRecDbl), hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < nIdx; k++) {
            if (spheres32) std::memcpy((SphereDbl*)spheres32 + k, &recs[k], sizeof(SphereDbl));
            if (primIdx) primIdx[k] = recs[k].prim;
        }
    }
    return 0;
}

}  // extern "C"
