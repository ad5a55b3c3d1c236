// sbvhbuild_host.cpp — the CPU twin of the device SBVH builder: BVH::BuildHQ of the reference (tiny_bvh.h:2623-3040, non-threaded) restated
// sequentially over sbvh_split.h.  Same loop, same slices, same double-buffered partition; BVH::Compact's numbering at the end (sbvhbuild.h).
#include "sbvhbuild.h"

#include <cstring>

#include "sbvh_split.h"

namespace tbvh {

namespace {
using sbvh::Frag;

struct HostSink {
    sbvh::AxisBins* ax;   // [3]
    void in(int a, int b) { ax[a].nin[b]++; }
    void out(int a, int b) { ax[a].nout[b]++; }
    void box(int a, int b, const float mn[3], const float mx[3]) {
        for (int k = 0; k < 3; k++) { ax[a].mn[b][k] = sah::min_ord(ax[a].mn[b][k], mn[k]); ax[a].mx[b][k] = sah::max_ord(ax[a].mx[b][k], mx[k]); }
    }
};

void clearBins(sbvh::AxisBins ax[3]) {
    for (int a = 0; a < 3; a++) for (int i = 0; i < sah::kBins; i++) {
        for (int k = 0; k < 3; k++) ax[a].mn[i][k] = sah::kFar, ax[a].mx[i][k] = -sah::kFar;
        ax[a].nin[i] = ax[a].nout[i] = 0;
    }
}

struct Task { uint32_t node, sliceStart, sliceEnd; };

void sbvh_split_leaves_host(const HostMesh& mesh, uint32_t k, std::vector<Node2>& nodes, const std::vector<uint32_t>& primIdx) {
    // as sah_build_host's SplitLeafs step (pairs behind the built nodes in the order of the leaves they split, leaf order kept), but every new node's
    // box is the bounds of its triangles INTERSECTED with the leaf's box: a leaf a spatial split has clipped must not grow back
    const uint32_t built = (uint32_t)nodes.size();
    uint32_t used = built;
    for (uint32_t i = 0; i < built; i++) {
        const uint32_t pairs = sah::split_leaf_pairs(nodes[i].triCount, k);
        if (!pairs) continue;
        const uint32_t base = used, first = nodes[i].leftFirst, count = nodes[i].triCount;
        used += 2 * pairs;
        nodes.resize(used);
        const Node2 leaf = nodes[i];
        float smn[3] = {sah::kFar, sah::kFar, sah::kFar}, smx[3] = {-sah::kFar, -sah::kFar, -sah::kFar};
        uint32_t end = count;
        for (uint32_t j = pairs + 1; j-- > 0;) {
            float cmn[3] = {sah::kFar, sah::kFar, sah::kFar}, cmx[3] = {-sah::kFar, -sah::kFar, -sah::kFar};
            for (uint32_t q = j * k; q < end; q++) {
                const size_t t = primIdx[first + q];
                float mn[3], mx[3];
                sah::fragment_box(mesh.xyz(t, 0), mesh.xyz(t, 1), mesh.xyz(t, 2), mn, mx);
                for (int c = 0; c < 3; c++) { cmn[c] = sah::min_ord(cmn[c], mn[c]); cmx[c] = sah::max_ord(cmx[c], mx[c]); }
            }
            for (int c = 0; c < 3; c++) { cmn[c] = sah::max_ord(cmn[c], leaf.mn[c]); cmx[c] = sah::min_ord(cmx[c], leaf.mx[c]); }
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
}  // namespace

uint32_t sbvh_build_host(const HostMesh& mesh, uint32_t nTris, uint32_t maxLeafTris, std::vector<Node2>& nodesOut, std::vector<uint32_t>& primIdxOut,
                         sbvh::Stats* statsOut) {
    nodesOut.clear(); primIdxOut.clear();
    sbvh::Stats st;
    memset(&st, 0, sizeof(st));
    if (statsOut) *statsOut = st;
    if (nTris == 0) return 0;
    const uint32_t slack = nTris >> 1, cap = nTris + slack;
    std::vector<Node2> nodes((size_t)nTris * 3, Node2{});
    std::vector<uint32_t> primIdx(cap, 0u), idxTmp(cap, 0u);
    std::vector<Frag> frag(cap);
    Node2& root = nodes[0];
    for (int k = 0; k < 3; k++) root.mn[k] = sah::kFar, root.mx[k] = -sah::kFar;
    root.leftFirst = 0; root.triCount = nTris;
    for (uint32_t i = 0; i < nTris; i++) {
        Frag& f = frag[i];
        sah::fragment_box(mesh.xyz(i, 0), mesh.xyz(i, 1), mesh.xyz(i, 2), f.mn, f.mx);
        f.prim = i; f.clipped = 0;
        for (int k = 0; k < 3; k++) { root.mn[k] = sah::min_ord(root.mn[k], f.mn[k]); root.mx[k] = sah::max_ord(root.mx[k], f.mx[k]); }
        primIdx[i] = i;
    }
    const float rootArea = sbvh::area3(root.mx, root.mn);
    float minDim[3];
    for (int k = 0; k < 3; k++) minDim[k] = (root.mx[k] - root.mn[k]) * 1e-7f;
    auto fetch = [&](uint32_t prim, float v[3][3]) {
        for (int i = 0; i < 3; i++) { const float* p = mesh.xyz(prim, i); v[i][0] = p[0]; v[i][1] = p[1]; v[i][2] = p[2]; }
    };
    uint32_t newNodePtr = 2, nextFrag = nTris, nodeIdx = 0, sliceStart = 0, sliceEnd = cap;
    std::vector<Task> task;
    sbvh::AxisBins ax[3];
    for (;;) {
        for (;;) {
            Node2& node = nodes[nodeIdx];
            // the object split
            clearBins(ax);
            float rpd[3];
            for (int a = 0; a < 3; a++) rpd[a] = sah::bin_scale(node.mn[a], node.mx[a]);
            for (uint32_t i = 0; i < node.triCount; i++) {
                const Frag& f = frag[primIdx[node.leftFirst + i]];
                for (int a = 0; a < 3; a++) {
                    const int b = sah::bin_index(f.mn[a], f.mx[a], node.mn[a], rpd[a]);
                    for (int k = 0; k < 3; k++) { ax[a].mn[b][k] = sah::min_ord(ax[a].mn[b][k], f.mn[k]); ax[a].mx[b][k] = sah::max_ord(ax[a].mx[b][k], f.mx[k]); }
                    ax[a].nin[b]++; ax[a].nout[b]++;
                }
            }
            const float noSplitCost = (float)node.triCount * 1.0f, rSAV = 1.0f / sbvh::area3(node.mx, node.mn);
            sbvh::Best best;
            memset(&best, 0, sizeof(best));
            best.splitCost = noSplitCost;
            float unused = 0.f;
            for (int a = 0; a < 3; a++) if ((node.mx[a] - node.mn[a]) > minDim[a]) sbvh::sweep_axis(ax[a], a, rSAV, false, 0, unused, best);
            // the spatial split
            const int budget = (int)(sliceEnd - sliceStart);
            if (sbvh::spatial_eligible(best, noSplitCost, budget, node.triCount, rootArea)) {
                float minSplitCost = best.splitCost * 0.985f;
                clearBins(ax);
                HostSink sink{ax};
                for (int a = 0; a < 3; a++) if ((node.mx[a] - node.mn[a]) > minDim[a]) {
                    for (uint32_t i = 0; i < node.triCount; i++)
                        sbvh::spatial_bin_fragment(frag[primIdx[node.leftFirst + i]], node.mn, node.mx, minDim, a, fetch, sink);
                    st.budgetRefusals += sbvh::sweep_axis(ax[a], a, rSAV, true, budget, minSplitCost, best);
                }
            }
            if (best.splitCost >= noSplitCost) {
                for (uint32_t i = 0; i < node.triCount; i++) primIdx[node.leftFirst + i] = frag[primIdx[node.leftFirst + i]].prim;
                break;
            }
            uint32_t A = sliceStart, B = sliceEnd, src = node.leftFirst;
            if (best.spatial) {
                st.spatialSplits++;
                const float planeDist = sbvh::plane_dist(node.mn[best.axis], node.mx[best.axis]), rPlaneDist = 1.0f / planeDist, nodeMin = node.mn[best.axis];
                sbvh::Chain c;
                for (int k = 0; k < 3; k++) { c.lmin[k] = best.lmin[k]; c.lmax[k] = best.lmax[k]; c.rmin[k] = best.rmin[k]; c.rmax[k] = best.rmax[k]; }
                c.nl = best.nl; c.nr = best.nr; c.splitCost = best.splitCost;
                for (uint32_t i = 0; i < node.triCount; i++) {
                    const uint32_t fi = primIdx[src++];
                    int where = sbvh::classify(frag[fi], best.axis, best.pos, nodeMin, rPlaneDist);
                    if (where == sbvh::kStraddler) {
                        where = sbvh::unsplit_step(c, frag[fi].mn, frag[fi].mx, rSAV);
                        if (where == sbvh::kToLeft) st.unsplitLeft++; else if (where == sbvh::kToRight) st.unsplitRight++;
                    }
                    if (where == sbvh::kSplit) {
                        float v[3][3];
                        fetch(frag[fi].prim, v);
                        Frag p1, p2;
                        bool leftOK, rightOK;
                        if (frag[fi].clipped) st.clippedReclips++;
                        sbvh::split_frag(frag[fi], v, minDim, best.axis, c.lmax[best.axis], p1, p2, leftOK, rightOK);
                        if (leftOK && rightOK) {
                            st.fragmentSplits++;
                            const uint32_t nf = nextFrag++;
                            frag[fi] = p1; idxTmp[A++] = fi;
                            frag[nf] = p2; idxTmp[--B] = nf;
                            continue;
                        }
                        st.oneSidedSplits++;
                        where = leftOK ? sbvh::kToLeft : sbvh::kToRight;
                    }
                    if (where == sbvh::kToLeft) idxTmp[A++] = fi; else idxTmp[--B] = fi;
                }
                // "for spatial splits, we fully refresh the bounds"
                for (int k = 0; k < 3; k++) { best.lmin[k] = best.rmin[k] = sah::kFar; best.lmax[k] = best.rmax[k] = -sah::kFar; }
                for (uint32_t i = sliceStart; i < A; i++) for (int k = 0; k < 3; k++) {
                    best.lmin[k] = sah::min_ord(best.lmin[k], frag[idxTmp[i]].mn[k]); best.lmax[k] = sah::max_ord(best.lmax[k], frag[idxTmp[i]].mx[k]);
                }
                for (uint32_t i = B; i < sliceEnd; i++) for (int k = 0; k < 3; k++) {
                    best.rmin[k] = sah::min_ord(best.rmin[k], frag[idxTmp[i]].mn[k]); best.rmax[k] = sah::max_ord(best.rmax[k], frag[idxTmp[i]].mx[k]);
                }
            } else {
                const float r = rpd[best.axis], nmin = node.mn[best.axis];
                for (uint32_t i = 0; i < node.triCount; i++) {
                    const uint32_t fr = primIdx[src + i];
                    if ((uint32_t)sah::bin_index(frag[fr].mn[best.axis], frag[fr].mx[best.axis], nmin, r) <= best.pos) idxTmp[A++] = fr; else idxTmp[--B] = fr;
                }
            }
            // (only the two ends of the slice hold anything; the reference copies the gap between them as well)
            for (uint32_t i = sliceStart; i < A; i++) primIdx[i] = idxTmp[i];
            for (uint32_t i = B; i < sliceEnd; i++) primIdx[i] = idxTmp[i];
            const uint32_t leftCount = A - sliceStart, rightCount = sliceEnd - B;
            if (leftCount == 0 || rightCount == 0) {
                // the reference's "spatial split failed" path reads primIdx entries that may be stale scratch (sbvhbuild.h): here the node becomes a
                // leaf over its fragments where the partition put them, with the refreshed bounds
                st.failedPartitions++;
                node.leftFirst = leftCount ? sliceStart : B;
                node.triCount = leftCount + rightCount;
                for (uint32_t i = 0; i < node.triCount; i++) primIdx[node.leftFirst + i] = frag[primIdx[node.leftFirst + i]].prim;
                for (int k = 0; k < 3; k++) { node.mn[k] = sah::min_ord(best.lmin[k], best.rmin[k]); node.mx[k] = sah::max_ord(best.lmax[k], best.rmax[k]); }
                break;
            }
            const uint32_t n = newNodePtr;
            newNodePtr += 2;
            Node2& l = nodes[n]; Node2& rr = nodes[n + 1];
            for (int k = 0; k < 3; k++) { l.mn[k] = best.lmin[k]; l.mx[k] = best.lmax[k]; rr.mn[k] = best.rmin[k]; rr.mx[k] = best.rmax[k]; }
            l.leftFirst = sliceStart; l.triCount = leftCount;
            rr.leftFirst = B; rr.triCount = rightCount;
            node.leftFirst = n; node.triCount = 0;
            const uint32_t mid = (A + B) >> 1;
            task.push_back(Task{n + 1, mid, sliceEnd});
            nodeIdx = n; sliceEnd = mid;
        }
        if (task.empty()) break;
        nodeIdx = task.back().node; sliceStart = task.back().sliceStart; sliceEnd = task.back().sliceEnd;
        task.pop_back();
    }
    // BVH::Compact (3733-3770): nodes in the pre-order of the interior nodes, leaves' entries consecutive from 0 in the order the walk meets them
    // (a root that stayed a leaf is left alone: two nodes, primIdx as it stands)
    if (nodes[0].triCount) {
        nodesOut.assign(nodes.begin(), nodes.begin() + 2);
        primIdxOut.assign(primIdx.begin(), primIdx.begin() + nodes[0].triCount);
    } else {
        nodesOut.assign(newNodePtr, Node2{});
        nodesOut[0] = nodes[0];
        uint32_t outPtr = 2, cur = 0;
        std::vector<uint32_t> stack;
        for (;;) {
            Node2& node = nodesOut[cur];
            if (node.triCount) {
                const uint32_t leafStart = (uint32_t)primIdxOut.size();
                for (uint32_t i = 0; i < node.triCount; i++) primIdxOut.push_back(primIdx[node.leftFirst + i]);
                node.leftFirst = leafStart;
                if (stack.empty()) break;
                cur = stack.back(); stack.pop_back();
            } else {
                nodesOut[outPtr] = nodes[node.leftFirst]; nodesOut[outPtr + 1] = nodes[node.leftFirst + 1];
                node.leftFirst = outPtr;
                stack.push_back(outPtr + 1);
                cur = outPtr;
                outPtr += 2;
            }
        }
    }
    st.refs = primIdxOut.size();
    if (maxLeafTris) sbvh_split_leaves_host(mesh, maxLeafTris, nodesOut, primIdxOut);
    if (statsOut) *statsOut = st;
    return (uint32_t)nodesOut.size();
}

}  // namespace tbvh
