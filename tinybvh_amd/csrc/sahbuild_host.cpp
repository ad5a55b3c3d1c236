// sahbuild_host.cpp — the CPU twin of the device SAH builder: BVH::Build( nodeIdx, depth ) of the reference (tiny_bvh.h:2332-2461, non-threaded)
// restated sequentially over sah_split.h.  Same loop, same node numbering; the leaves' primitives are sorted at the end (sahbuild.h).
#include "sahbuild.h"

#include <algorithm>
#include <cstring>

#include "sah_split.h"

namespace tbvh {

namespace {
struct HostBins {
    float mnv[3][sah::kBins][3], mxv[3][sah::kBins][3];
    uint32_t cnt[3][sah::kBins];
    float mn(int a, int i, int k) const { return mnv[a][i][k]; }
    float mx(int a, int i, int k) const { return mxv[a][i][k]; }
    uint32_t count(int a, int i) const { return cnt[a][i]; }
    void clear() {
        for (int a = 0; a < 3; a++) for (int i = 0; i < sah::kBins; i++) {
            for (int k = 0; k < 3; k++) mnv[a][i][k] = sah::kFar, mxv[a][i][k] = -sah::kFar;
            cnt[a][i] = 0;
        }
    }
};
}  // namespace

// Build() over filled fragments: everything after the fragment step (the root box included, taken in the order of sah::key)
static uint32_t build_fragments(const std::vector<float>& fmn, const std::vector<float>& fmx, uint32_t nTris, uint32_t maxLeafTris, std::vector<Node2>& nodes,
                                std::vector<uint32_t>& primIdx) {
    nodes.assign((size_t)nTris * 2, Node2{});   // (node 1 stays zero)
    primIdx.resize(nTris);
    Node2& root = nodes[0];
    for (int k = 0; k < 3; k++) root.mn[k] = sah::kFar, root.mx[k] = -sah::kFar;
    root.leftFirst = 0; root.triCount = nTris;
    for (uint32_t i = 0; i < nTris; i++) {
        for (int k = 0; k < 3; k++) {
            root.mn[k] = sah::min_ord(root.mn[k], fmn[3 * (size_t)i + k]);
            root.mx[k] = sah::max_ord(root.mx[k], fmx[3 * (size_t)i + k]);
        }
        primIdx[i] = i;
    }
    float minDim[3];
    for (int k = 0; k < 3; k++) minDim[k] = (root.mx[k] - root.mn[k]) * 1e-20f;
    uint32_t newNodePtr = 2, nodeIdx = 0;
    std::vector<uint32_t> task;
    HostBins bins;
    for (;;) {
        for (;;) {
            Node2& node = nodes[nodeIdx];
            bins.clear();
            float rpd[3];
            for (int a = 0; a < 3; a++) rpd[a] = sah::bin_scale(node.mn[a], node.mx[a]);
            for (uint32_t i = 0; i < node.triCount; i++) {
                const size_t fi = primIdx[node.leftFirst + i];
                const float* bmn = &fmn[3 * fi]; const float* bmx = &fmx[3 * fi];
                for (int a = 0; a < 3; a++) {
                    const int b = sah::bin_index(bmn[a], bmx[a], node.mn[a], rpd[a]);
                    for (int k = 0; k < 3; k++) {
                        bins.mnv[a][b][k] = sah::min_ord(bins.mnv[a][b][k], bmn[k]);
                        bins.mxv[a][b][k] = sah::max_ord(bins.mxv[a][b][k], bmx[k]);
                    }
                    bins.cnt[a][b]++;
                }
            }
            sah::Split s;
            if (!sah::find_split(bins, node.mn, node.mx, minDim, node.triCount, nodeIdx == 0, s)) break;
            const uint32_t leftCount = sah::left_count(bins, s), rightCount = node.triCount - leftCount;
            if (leftCount == 0 || rightCount == 0) break;
            // partition: the order inside the two halves is free (the leaves are sorted at the end)
            uint32_t* first = &primIdx[node.leftFirst];
            const float nmin = node.mn[s.axis], r = rpd[s.axis];
            std::partition(first, first + node.triCount, [&](uint32_t fi) {
                return (uint32_t)sah::bin_index(fmn[3 * (size_t)fi + s.axis], fmx[3 * (size_t)fi + s.axis], nmin, r) <= s.pos;
            });
            const uint32_t n = newNodePtr;
            newNodePtr += 2;
            Node2& l = nodes[n]; Node2& rr = nodes[n + 1];
            for (int k = 0; k < 3; k++) { l.mn[k] = s.lmin[k]; l.mx[k] = s.lmax[k]; rr.mn[k] = s.rmin[k]; rr.mx[k] = s.rmax[k]; }
            l.leftFirst = node.leftFirst; l.triCount = leftCount;
            rr.leftFirst = node.leftFirst + leftCount; rr.triCount = rightCount;
            node.leftFirst = n; node.triCount = 0;
            task.push_back(n + 1);
            nodeIdx = n;
        }
        if (task.empty()) break;
        nodeIdx = task.back(); task.pop_back();
    }
    uint32_t used = newNodePtr;
    for (uint32_t i = 0; i < used; i++)
        if (nodes[i].triCount) std::sort(&primIdx[nodes[i].leftFirst], &primIdx[nodes[i].leftFirst] + nodes[i].triCount);
    if (maxLeafTris) {
        // SplitLeafs: the pairs of leaf i follow those of every leaf with a smaller index (the device builder's exclusive scan over the nodes); pair j
        // holds primitives [j k, j k + k) on the left and the rest on the right, every new node with the bounds of its own primitives, written from
        // the last pair to the first (kernels_sahbuild.hip: k_sah_split_emit)
        const uint32_t built = used, k = maxLeafTris;
        for (uint32_t i = 0; i < built; i++) {
            const uint32_t pairs = sah::split_leaf_pairs(nodes[i].triCount, k);
            if (!pairs) continue;
            const uint32_t base = used, first = nodes[i].leftFirst, count = nodes[i].triCount;
            used += 2 * pairs;
            if ((size_t)used > nodes.size()) nodes.resize(used);
            float smn[3] = {sah::kFar, sah::kFar, sah::kFar}, smx[3] = {-sah::kFar, -sah::kFar, -sah::kFar};
            uint32_t end = count;
            for (uint32_t j = pairs + 1; j-- > 0;) {
                float cmn[3] = {sah::kFar, sah::kFar, sah::kFar}, cmx[3] = {-sah::kFar, -sah::kFar, -sah::kFar};
                for (uint32_t q = j * k; q < end; q++) {
                    const size_t fi = primIdx[first + q];
                    for (int c = 0; c < 3; c++) { cmn[c] = sah::min_ord(cmn[c], fmn[3 * fi + c]); cmx[c] = sah::max_ord(cmx[c], fmx[3 * fi + c]); }
                }
                if (j < pairs) {
                    const uint32_t at = base + 2 * j;
                    const bool last = j == pairs - 1;
                    Node2& l = nodes[at]; Node2& r = nodes[at + 1];
                    for (int c = 0; c < 3; c++) { l.mn[c] = cmn[c]; l.mx[c] = cmx[c]; r.mn[c] = smn[c]; r.mx[c] = smx[c]; }
                    l.leftFirst = first + j * k; l.triCount = k;
                    r.leftFirst = last ? first + (j + 1) * k : at + 2; r.triCount = last ? count - (j + 1) * k : 0;
                }
                for (int c = 0; c < 3; c++) { smn[c] = sah::min_ord(smn[c], cmn[c]); smx[c] = sah::max_ord(smx[c], cmx[c]); }
                end = j * k;
            }
            nodes[i].leftFirst = base; nodes[i].triCount = 0;
        }
    }
    nodes.resize(used);
    return used;
}

uint32_t sah_build_host(const HostMesh& mesh, uint32_t nTris, uint32_t maxLeafTris, std::vector<Node2>& nodes, std::vector<uint32_t>& primIdx) {
    nodes.clear(); primIdx.clear();
    if (nTris == 0) return 0;
    std::vector<float> fmn((size_t)nTris * 3), fmx((size_t)nTris * 3);
    for (uint32_t i = 0; i < nTris; i++) sah::fragment_box(mesh.xyz(i, 0), mesh.xyz(i, 1), mesh.xyz(i, 2), &fmn[3 * (size_t)i], &fmx[3 * (size_t)i]);
    return build_fragments(fmn, fmx, nTris, maxLeafTris, nodes, primIdx);
}

uint32_t sah_build_host(const SahBoxes& boxes, uint32_t n, uint32_t maxLeaf, std::vector<Node2>& nodes, std::vector<uint32_t>& primIdx) {
    nodes.clear(); primIdx.clear();
    if (n == 0) return 0;
    std::vector<float> fmn((size_t)n * 3), fmx((size_t)n * 3);
    for (uint32_t i = 0; i < n; i++) {
        const float* rec = boxes.data + (size_t)i * boxes.stride;
        if (boxes.spheres) sah::sphere_box(rec, &fmn[3 * (size_t)i], &fmx[3 * (size_t)i]);
        else for (int k = 0; k < 3; k++) { fmn[3 * (size_t)i + k] = rec[boxes.offMin + k]; fmx[3 * (size_t)i + k] = rec[boxes.offMax + k]; }
    }
    return build_fragments(fmn, fmx, n, maxLeaf, nodes, primIdx);
}

}  // namespace tbvh
