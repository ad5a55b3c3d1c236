"""Structural check of a single-precision BLAS blob against the caller's triangles: decode every node, walk the tree level by level and compare every
stored child box with the exact float32 box of the triangles beneath it.  Min and max are exact in float, so the truth needs no tolerance; only the two
quantised layouts have a (derived, not measured) bound on how far OUTSIDE the truth a plane may lie.

check_tree() reports, assert_tree() judges.  numpy only; one pass of array operations per tree level, nothing per node.

Layouts (all blobs as (n, 4) uint32 arrays of 16-byte blocks, as Scene.download_blobs() / HostBVH.blob() return them):
  LAYOUT_BVH_GPU   64-byte nodes {lmin,left | lmax,right | rmin,triCount | rmax,firstTri}; `tris` is either the gathered records {v0|prim, e1, e2}
                   (a downloaded scene) or the primIdx array of width 1 (a host blob: no records to compare then).
  LAYOUT_BVH4_GPU  one stream: node = {bmin | qxmin[4]} {e255 | qxmax[4]} {qymin qymax qzmin qzmax} {childInfo[4]}, plane = bmin + e255 * q, the records
                   {v0|prim, e1, e2} of leaf children inline; childInfo 0 = empty, bit 31 = leaf (count << 16 | rel), else a node's block offset.
  LAYOUT_CWBVH     80-byte nodes {lo, e[3] | imask << 24} {childBase, triBase, meta[8]} {qlo_x qlo_y qlo_z qhi_x qhi_y qhi_z, 8 bytes each},
                   plane = lo + 2^e * q, records {e2, e1, v0|prim}.
The encoders are compiled without contraction, so a plane is a rounded float32 product followed by a rounded float32 sum: what numpy computes."""
import numpy as np

LAYOUT_BVH_GPU, LAYOUT_BVH4_GPU, LAYOUT_CWBVH = 5, 8, 10

# ---- bounds on the outward slack of a quantised plane, in units of the node's step (2^e or e255) ------------------------------------------
# Derived from the encoders' rules: the encoder takes the tightest conservative quantum (floor / ceil: less than one step) and one more step can
# be lost to the rounding of origin + q * step; BVH4_GPU pads every plane by guard = 4e-7 * max(|bmin|, |bmax|, ext) before choosing the quantum,
# once for the frame (e255 carries 255 steps to bmax + guard) and once for the plane itself.
# Host encoder's own maxima (test_host_built_trees_pass prints them; soup 3000, blob 8000, soup 2000 far from the origin, a flat soup, 1 and 9
# triangles, whole-triangle builds): CWBVH 1.000 steps, exponent excess 0, "+ 1" used 0 times; BVH4_GPU 1.032 (e255 + guard), reached far from the origin where the guard is a few ulps.
CWBVH_SLACK_STEPS = 2.0
CWBVH_EXPONENT_EXCESS = 1
BVH4_SLACK_STEPS = 2.0          # in units of e255 + guard, i.e. 2 + 2 * guard / e255 steps
BVH4_GUARD = 4e-7

_INF = np.float32(np.inf)


def _f32(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def _bytes4(w):
    """(..., ) uint32 -> (..., 4) the four bytes, least significant first"""
    return np.stack([(w >> np.uint32(8 * k)) & np.uint32(255) for k in range(4)], -1)


def _popcount(x):
    x = x.astype(np.uint32)
    c = np.zeros(x.shape, np.uint32)
    for k in range(8):
        c += (x >> np.uint32(k)) & np.uint32(1)
    return c


def triangles(verts, indices=None):
    """(n, 3, 4) float32: the three bvhvec4 of every triangle (w = 0 where the vertex array has no fourth column)."""
    v = np.asarray(verts, np.float32)
    if indices is None and v.ndim == 2 and v.shape[1] == 4:
        return v.reshape(-1, 3, 4)
    if v.shape[1] < 4 or v.strides[0] != 16:
        v = np.concatenate([v[:, :3], np.zeros((v.shape[0], 1), np.float32)], 1)
    if indices is None:
        return np.ascontiguousarray(v).reshape(-1, 3, 4)
    return v[np.asarray(indices, np.int64).reshape(-1, 3)]


def expected_records(layout, tri):
    """(n, 3, 4) uint32: the record of every triangle in the layout's order, {v0|prim, v1 - v0, v2 - v0} computed in float32."""
    n = tri.shape[0]
    a = tri[:, 0].copy(); a.view(np.uint32)[:, 3] = np.arange(n, dtype=np.uint32)
    e1 = tri[:, 1] - tri[:, 0]; e2 = tri[:, 2] - tri[:, 0]
    rec = np.stack([e2, e1, a], 1) if layout == LAYOUT_CWBVH else np.stack([a, e1, e2], 1)
    return np.ascontiguousarray(rec).view(np.uint32)


class _Blob:
    """The layout-specific part: decode(ids) -> per node and slot what the walk needs."""

    def __init__(self, layout, nodes, tris):
        self.layout = layout
        self.u = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 4)
        t = np.ascontiguousarray(tris, np.uint32) if tris is not None else np.zeros((0, 4), np.uint32)
        self.prim_only = layout == LAYOUT_BVH_GPU and (t.ndim == 1 or t.shape[-1] == 1)
        if layout == LAYOUT_BVH4_GPU:
            self.n_ids = self.u.shape[0]                      # a node id is its block offset
            self.rec_blocks = self.u                          # records live in the stream; a record id is its block offset
            self.n_rec_blocks = self.u.shape[0]
        else:
            self.n_ids = self.u.shape[0] // (5 if layout == LAYOUT_CWBVH else 4)
            if self.prim_only:
                self.prim_idx = t.reshape(-1)
                self.n_rec_blocks = 3 * self.prim_idx.size
            else:
                self.rec_blocks = t.reshape(-1, 4)
                self.n_rec_blocks = self.rec_blocks.shape[0]
        self.slots = {LAYOUT_BVH_GPU: 2, LAYOUT_BVH4_GPU: 4, LAYOUT_CWBVH: 8}[layout]
        self.prim_block = 2 if layout == LAYOUT_CWBVH else 0    # which block of a record carries the prim word
        self.record_stride = 3 if layout == LAYOUT_BVH4_GPU else 1   # from one record id to the next (BVH4_GPU: ids are block offsets)

    def root_ok(self):
        return self.u.shape[0] >= (5 if self.layout == LAYOUT_CWBVH else 4)

    def record_block(self, rec):
        """first block of record id `rec`"""
        return rec if self.layout == LAYOUT_BVH4_GPU else 3 * rec

    def prims_of(self, rec):
        if self.prim_only:
            return self.prim_idx[rec]
        return self.rec_blocks[self.record_block(rec) + self.prim_block, 3]

    def records_of(self, rec):
        b = self.record_block(rec)
        return np.stack([self.rec_blocks[b], self.rec_blocks[b + 1], self.rec_blocks[b + 2]], 1)

    def decode(self, ids):
        ids = np.asarray(ids, np.int64)
        N, S = ids.size, self.slots
        d = {"ids": ids}
        if self.layout == LAYOUT_BVH_GPU:
            w = self.u.reshape(-1, 16)[ids]
            f = _f32(w)
            child = np.stack([w[:, 3], w[:, 7]], 1).astype(np.int64)
            d["plo"] = np.stack([f[:, 0:3], f[:, 8:11]], 1); d["phi"] = np.stack([f[:, 4:7], f[:, 12:15]], 1)
            in_range = child < self.n_ids
            cw = self.u.reshape(-1, 16)[np.where(in_range, child, 0)]
            d["valid"] = np.ones((N, S), bool)
            d["child_ok"] = in_range
            d["interior"] = in_range & (cw[..., 11] == 0)
            d["child"] = child
            d["count"] = np.where(in_range, cw[..., 11], 0).astype(np.int64)
            d["first"] = cw[..., 15].astype(np.int64)
            d["leaf_node"] = in_range & (cw[..., 11] != 0)       # a leaf child is a node of its own here
            d["step"] = None
            return d
        if self.layout == LAYOUT_BVH4_GPU:
            b = self.u[ids[:, None] + np.arange(4)[None, :]]      # (N, 4 blocks, 4 words)
            f = _f32(b)
            org, step = f[:, 0, :3], f[:, 1, :3]
            q = np.stack([_bytes4(b[:, 0, 3]), _bytes4(b[:, 1, 3]), _bytes4(b[:, 2, 0]), _bytes4(b[:, 2, 1]), _bytes4(b[:, 2, 2]), _bytes4(b[:, 2, 3])], -1)  # (N, child, 6)
            qlo, qhi = q[..., 0::2], q[..., 1::2]
            info = b[:, 3, :]
            d["valid"] = info != 0
            leaf = (info >> np.uint32(31)) != 0
            d["interior"] = d["valid"] & ~leaf
            d["child"] = info.astype(np.int64)
            d["child_ok"] = ~d["interior"] | (d["child"] + 4 <= self.n_ids)
            d["count"] = np.where(leaf, (info >> np.uint32(16)) & np.uint32(0x7fff), 0).astype(np.int64)
            d["first"] = ids[:, None] + (info & np.uint32(0xffff)).astype(np.int64)
        else:
            b = self.u.reshape(-1, 5, 4)[ids]
            f = _f32(b)
            org = f[:, 0, :3]
            ew = b[:, 0, 3]
            e = _bytes4(ew)[:, :3].astype(np.uint8).view(np.int8).astype(np.int32)
            imask = (ew >> np.uint32(24)).astype(np.uint32)
            step = np.ldexp(np.float32(1), e).astype(np.float32)
            meta = np.concatenate([_bytes4(b[:, 1, 2]), _bytes4(b[:, 1, 3])], 1)          # (N, 8)
            planes = b[:, 2:5, :].reshape(N, 6, 2)                                          # six 8-byte arrays
            q8 = np.concatenate([_bytes4(planes[:, :, 0]), _bytes4(planes[:, :, 1])], -1)   # (N, 6, 8 slots)
            qlo, qhi = np.moveaxis(q8[:, 0:3, :], 1, 2), np.moveaxis(q8[:, 3:6, :], 1, 2)   # (N, slot, axis)
            sl = np.arange(8, dtype=np.uint32)[None, :]
            d["valid"] = meta != 0
            d["interior"] = d["valid"] & (((imask[:, None] >> sl) & 1) != 0)
            below = imask[:, None] & ((np.uint32(1) << sl) - np.uint32(1))
            d["child"] = b[:, 1, 0].astype(np.int64)[:, None] + _popcount(below).astype(np.int64)
            d["child_ok"] = ~d["interior"] | (d["child"] < self.n_ids)
            d["count"] = np.where(d["valid"] & ~d["interior"], _popcount(meta >> np.uint32(5)), 0).astype(np.int64)
            d["first"] = (b[:, 1, 1] // np.uint32(3)).astype(np.int64)[:, None] + (meta & np.uint32(31)).astype(np.int64)
            d["e"] = e
        d["origin"], d["step"] = org, step
        d["qlo"], d["qhi"] = qlo.astype(np.int32), qhi.astype(np.int32)
        d["plo"] = org[:, None, :] + step[:, None, :] * qlo.astype(np.float32)              # float32: rounded product, rounded sum
        d["phi"] = org[:, None, :] + step[:, None, :] * qhi.astype(np.float32)
        return d


def check_tree(layout, nodes, tris, verts, indices=None):
    """Findings about the blob (nodes, tris) of `layout` over the caller's triangles; asserts nothing.  Keys:
      nodes_reached, prims (every prim word reached, with multiplicity), bad_index / multi_reached / record_mismatch / containment / inexact /
      short_reach / slack_over / exponent_over / step_over: lists of findings (tuples that start with node, slot, axis where they apply), max_slack (largest
      outward distance of a plane in units of the node's step, for BVH4_GPU of step + guard) and max_slack_at, exponent_plus_one (how often a CWBVH exponent is one
      above the minimum), and `planes`: one row per stored child box (node, slot, plo, phi, tlo, thi, slack_lo, slack_hi, qlo, qhi, step) for
      the tests that look for a particular plane."""
    blob = _Blob(layout, nodes, tris)
    tri = triangles(verts, indices)
    n_tris = tri.shape[0]
    tmin, tmax = tri[:, :, :3].min(1), tri[:, :, :3].max(1)
    want_rec = None if blob.prim_only else expected_records(layout, tri)
    F = {"layout": layout, "bad_index": [], "multi_reached": [], "record_mismatch": [], "containment": [], "inexact": [], "short_reach": [],
         "slack_over": [], "exponent_over": [], "step_over": [], "exponent_plus_one": 0, "exponent_count": 0, "max_slack": 0.0, "max_slack_at": None,
         "nodes_reached": 0, "levels": 0, "records_compared": 0}
    prims = []
    rows = {k: [] for k in ("node", "slot", "plo", "phi", "tlo", "thi", "qlo", "qhi", "step", "guard")}
    if not blob.root_ok():
        F["bad_index"].append((0, -1, "no root"))
        F["prims"] = np.zeros(0, np.uint32); F["planes"] = None
        return F
    # a BVH_GPU whose root is a leaf: nothing but its triangles
    if layout == LAYOUT_BVH_GPU and blob.u.reshape(-1, 16)[0, 11] != 0:
        cnt, first = int(blob.u.reshape(-1, 16)[0, 11]), int(blob.u.reshape(-1, 16)[0, 15])
        rec = np.arange(first, first + cnt)
        if 3 * (first + cnt) > blob.n_rec_blocks:
            F["bad_index"].append((0, -1, "leaf records beyond the array"))
            rec = rec[:0]
        p = blob.prims_of(rec)
        if want_rec is not None:
            ok = p < n_tris
            bad = np.any(blob.records_of(rec[ok]) != want_rec[p[ok]], axis=(1, 2))
            F["record_mismatch"] += [(0, -1, int(r)) for r in rec[ok][bad]]
            F["records_compared"] += int(ok.sum())
        F["prims"] = p.astype(np.uint32); F["nodes_reached"] = 1; F["planes"] = None
        return F

    # ---- top-down: the nodes of every level, each expanded the first time it is reached ------------------------------------------------
    seen = np.zeros(blob.n_ids, np.uint8)
    seen[0] = 1
    levels = []
    frontier = np.zeros(1, np.int64)
    while frontier.size:
        d = blob.decode(frontier)
        levels.append(d)
        bad = d["valid"] & ~d["child_ok"]
        for n, s in zip(*np.nonzero(bad)):
            F["bad_index"].append((int(frontier[n]), int(s), f"child {int(d['child'][n, s])} beyond the array"))
        d["interior"] &= d["child_ok"]
        d["valid"] &= d["child_ok"]
        # leaf record ranges
        leaf = d["valid"] & ~d["interior"]
        end_block = blob.record_block(d["first"]) + 3 * d["count"]
        over = leaf & (end_block > blob.n_rec_blocks)
        for n, s in zip(*np.nonzero(over)):
            F["bad_index"].append((int(frontier[n]), int(s), "leaf records beyond the array"))
        d["count"] = np.where(over, 0, d["count"])
        # nodes reached: interior children, and for BVH_GPU the leaf nodes too
        reach = d["interior"] | d.get("leaf_node", False) & d["valid"]
        c = d["child"][reach]
        uniq, cnt = np.unique(c, return_counts=True)
        again = uniq[(cnt > 1) | (seen[uniq] != 0)]
        F["multi_reached"] += [int(x) for x in again]
        ci = d["child"][d["interior"]]
        nxt = np.unique(ci[seen[ci] == 0])
        seen[uniq] = 1
        frontier = nxt
        if len(levels) > 100000:
            F["bad_index"].append((int(frontier[0]) if frontier.size else 0, -1, "more than 100000 levels"))
            break
    F["levels"] = len(levels)
    F["nodes_reached"] = int(seen.sum())

    # ---- bottom-up: the truth of every child, the union for the node ------------------------------------------------------------------------
    node_lo = np.full((blob.n_ids, 3), _INF, np.float32)
    node_hi = np.full((blob.n_ids, 3), -_INF, np.float32)
    for d in reversed(levels):
        ids = d["ids"]
        N, S = d["valid"].shape
        tlo = np.full((N, S, 3), _INF, np.float32); thi = np.full((N, S, 3), -_INF, np.float32)
        m = d["interior"]
        tlo[m] = node_lo[d["child"][m]]; thi[m] = node_hi[d["child"][m]]
        leaf = d["valid"] & ~d["interior"]
        for k in range(int(d["count"].max()) if d["count"].size else 0):
            mk = leaf & (d["count"] > k)
            rec = d["first"][mk] + blob.record_stride * k
            p = blob.prims_of(rec)
            prims.append(p)
            ok = p < n_tris
            nn, ss = np.nonzero(mk)
            for n, s in zip(nn[~ok], ss[~ok]):
                F["bad_index"].append((int(ids[n]), int(s), "prim beyond the triangles"))
            nn, ss, rec, p = nn[ok], ss[ok], rec[ok], p[ok].astype(np.int64)
            tlo[nn, ss] = np.minimum(tlo[nn, ss], tmin[p]); thi[nn, ss] = np.maximum(thi[nn, ss], tmax[p])
            if want_rec is not None:
                badrec = np.any(blob.records_of(rec) != want_rec[p], axis=(1, 2))
                F["record_mismatch"] += [(int(ids[n]), int(s), int(r)) for n, s, r in zip(nn[badrec], ss[badrec], rec[badrec])]
                F["records_compared"] += int(rec.size)
        node_lo[ids] = tlo.min(1); node_hi[ids] = thi.max(1)
        d["tlo"], d["thi"] = tlo, thi

    # ---- compare ----------------------------------------------------------------------------------------------------------------------------------
    for d in levels:
        ids = d["ids"]
        known = d["valid"] & np.all(d["tlo"] <= d["thi"], -1)          # children whose truth is not empty
        nn, ss = np.nonzero(known)
        if nn.size == 0:
            continue
        plo, phi, tlo, thi = d["plo"][nn, ss], d["phi"][nn, ss], d["tlo"][nn, ss], d["thi"][nn, ss]
        for side, badm in (("lo", plo > tlo), ("hi", phi < thi)):
            for r, a in zip(*np.nonzero(badm)):
                F["containment"].append((int(ids[nn[r]]), int(ss[r]), int(a), side, float((plo if side == "lo" else phi)[r, a]), float((tlo if side == "lo" else thi)[r, a])))
        rows["node"].append(ids[nn]); rows["slot"].append(ss)
        rows["plo"].append(plo); rows["phi"].append(phi); rows["tlo"].append(tlo); rows["thi"].append(thi)
        if layout == LAYOUT_BVH_GPU:
            for side, st, tr in (("lo", plo, tlo), ("hi", phi, thi)):
                for r, a in zip(*np.nonzero(st.view(np.uint32) != tr.view(np.uint32))):
                    F["inexact"].append((int(ids[nn[r]]), int(ss[r]), int(a), side, float(st[r, a]), float(tr[r, a])))
            continue
        # the node's own truth, its origin and its step
        nlo, nhi = node_lo[ids], node_hi[ids]
        has = np.all(nlo <= nhi, -1)
        for n, a in zip(*np.nonzero((d["origin"].view(np.uint32) != nlo.view(np.uint32)) & has[:, None])):
            F["inexact"].append((int(ids[n]), -1, int(a), "origin", float(d["origin"][n, a]), float(nlo[n, a])))
        reach = d["origin"] + d["step"] * np.float32(255)
        for n, a in zip(*np.nonzero((reach < nhi) & has[:, None])):
            F["short_reach"].append((int(ids[n]), -1, int(a), float(reach[n, a]), float(nhi[n, a])))
        ext = nhi - nlo                                                 # float32, as the encoders take it
        if layout == LAYOUT_CWBVH:
            with np.errstate(divide="ignore", invalid="ignore"):
                emin = np.where(ext > 0, np.ceil(np.log2(ext.astype(np.float64) / 255.0)), -126.0)
            emin = np.maximum(emin, -126.0).astype(np.int32)
            excess = np.where(has[:, None], d["e"] - emin, 0)
            F["exponent_plus_one"] += int((excess == 1).sum())
            F["exponent_count"] += int(has.sum()) * 3
            for n, a in zip(*np.nonzero(excess > CWBVH_EXPONENT_EXCESS)):
                F["exponent_over"].append((int(ids[n]), -1, int(a), int(d["e"][n, a]), int(emin[n, a])))
            guard = np.zeros_like(ext)
        else:
            guard = np.float32(BVH4_GUARD) * np.maximum(np.maximum(np.abs(nlo), np.abs(nhi)), ext)
            # the step itself must be tight, or a stale large e255 would make every plane look close in ITS units: bvh4_frame carries 255 steps to
            # bmax + guard and stops at the first float that gets there, so the reach ends below bmax + 2 guard (the rounding of the few sums
            # involved is a fraction of the guard, which is 3 to 7 ulps of the largest coordinate); no extent, no step
            far_ok = np.where(ext > 0, reach.astype(np.float64) <= nhi.astype(np.float64) + 2.0 * guard.astype(np.float64), d["step"] == 0)
            for n, a in zip(*np.nonzero(~far_ok & has[:, None])):
                F["step_over"].append((int(ids[n]), -1, int(a), float(d["step"][n, a]), float(ext[n, a])))
        # outward slack in units of step + guard (guard = 0 for CWBVH): out < 2 (step + guard) is the issue's "slack < 2 + 2 guard / e255 steps"
        unit = d["step"][nn].astype(np.float64) + guard[nn].astype(np.float64)
        out = np.stack([tlo.astype(np.float64) - plo.astype(np.float64), phi.astype(np.float64) - thi.astype(np.float64)], -1)   # (rows, axis, side)
        with np.errstate(divide="ignore", invalid="ignore"):
            slack = np.where(out > 0, out / unit[..., None], 0.0)
        bound = CWBVH_SLACK_STEPS if layout == LAYOUT_CWBVH else BVH4_SLACK_STEPS
        for r, a, sd in zip(*np.nonzero(~(slack < bound))):
            F["slack_over"].append((int(ids[nn[r]]), int(ss[r]), int(a), ("lo", "hi")[sd], float(slack[r, a, sd]), float(bound)))
        if float(slack.max()) > F["max_slack"]:
            r, a, sd = np.unravel_index(int(np.argmax(slack)), slack.shape)
            F["max_slack"] = float(slack[r, a, sd]); F["max_slack_at"] = (int(ids[nn[r]]), int(ss[r]), int(a), ("lo", "hi")[sd])
        rows["qlo"].append(d["qlo"][nn, ss]); rows["qhi"].append(d["qhi"][nn, ss]); rows["step"].append(d["step"][nn]); rows["guard"].append(guard[nn])
    F["prims"] = np.concatenate(prims).astype(np.uint32) if prims else np.zeros(0, np.uint32)
    F["planes"] = {k: np.concatenate(v) for k, v in rows.items() if v}
    if "step" in F["planes"]:
        P = F["planes"]
        with np.errstate(divide="ignore", invalid="ignore"):
            st = P["step"].astype(np.float64)
            P["slack_lo"] = np.where(P["tlo"] > P["plo"], (P["tlo"].astype(np.float64) - P["plo"]) / st, 0.0)
            P["slack_hi"] = np.where(P["phi"] > P["thi"], (P["phi"].astype(np.float64) - P["thi"]) / st, 0.0)
    F["node_truth"] = (node_lo, node_hi)
    return F


def describe(F):
    """One line per tree for the logs: what the pull request text reports."""
    return (f"layout {F['layout']}: {F['nodes_reached']} nodes, {F['levels']} levels, {F['prims'].size} prims, containment {len(F['containment'])}, "
            f"inexact {len(F['inexact'])}, max slack {F['max_slack']:.3f} " + ("(step + guard)" if F["layout"] == LAYOUT_BVH4_GPU else "steps")
            + (f", exponent +1 used {F['exponent_plus_one']} of {F['exponent_count']}" if F["layout"] == LAYOUT_CWBVH else ""))


def _first(kind, items):
    it = items[0]
    return f"{kind}: {len(items)} finding(s), first at node {it[0]}, slot {it[1]}, axis {it[2] if len(it) > 2 else '-'}: {it}"


def assert_tree(layout, nodes, tris, verts, indices=None, prims=None, label=""):
    """check_tree + the conditions: topology (every node once, no index outside the arrays, the multiset of prim words = `prims`, default every
    triangle once), records bit-equal, containment with zero tolerance, exact float boxes / origins, slack and exponent within the derived bounds.
    Returns the findings."""
    F = check_tree(layout, nodes, tris, verts, indices)
    where = f"[{label}] " if label else ""
    assert not F["bad_index"], where + _first("index outside the arrays", F["bad_index"])
    assert not F["multi_reached"], where + f"nodes reached more than once: {F['multi_reached'][:8]}"
    want = np.arange(triangles(verts, indices).shape[0], dtype=np.uint32) if prims is None else np.sort(np.asarray(prims, np.uint32).reshape(-1))
    got = np.sort(F["prims"])
    if got.size != want.size or not np.array_equal(got, want):
        missing = np.setdiff1d(want, got)[:8]; extra = np.setdiff1d(got, want)[:8]
        raise AssertionError(where + f"prims reached: {got.size}, expected {want.size}; missing {missing}, unexpected {extra}")
    assert not F["record_mismatch"], where + _first("triangle record differs from {v0|prim, v1 - v0, v2 - v0}", F["record_mismatch"])
    assert not F["containment"], where + _first("child plane inside the truth", F["containment"])
    assert not F["short_reach"], where + _first("255 steps stop short of the far face", F["short_reach"])
    assert not F["inexact"], where + _first("stored float differs from the truth", F["inexact"])
    assert not F["exponent_over"], where + _first("exponent above the minimum + 1", F["exponent_over"])
    assert not F["step_over"], where + _first("BVH4_GPU step carries 255 steps beyond bmax + 2 guard", F["step_over"])
    assert not F["slack_over"], where + _first("plane too far outside the truth", F["slack_over"])
    return F
