"""Shared helpers for the parity tests: run the HIP engine and the CPU oracle on the same cloud and
compare stage by stage (P0 exact integer stages, P1 float attributes, P2 partition)."""
import numpy as np


def oracle_params(oracle, p, **kw):
    """RefParams from a VgsParams (same Task-file values); math=1 DevMath / flavour=1 lean by default."""
    d = dict(voxel_size=p.voxel_size, graph_size=p.graph_size, sig_p=p.sig_p, sig_n=p.sig_n, sig_o=p.sig_o, sig_e=p.sig_e,
             sig_c=p.sig_c, sig_w=p.sig_w, cut_thred=p.cut_thred, points_min=p.points_min, adjacency_min=p.adjacency_min,
             voxels_min=p.voxels_min, seed_size=p.seed_size, color_impt=p.color_impt, spatial_impt=p.spatial_impt,
             normal_impt=p.normal_impt, q7_count_as_index=p.q7_count_as_index, math=1, flavour=1)
    d.update(kw)
    return oracle.vgs_params(**d)


def ragged_sets(off, idx):
    return [frozenset(idx[off[i]:off[i + 1]].tolist()) for i in range(len(off) - 1)]


def ragged_lists(off, idx):
    return [idx[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


def partition_agreement(a, b):
    """Fraction of elements whose segment in `a` is matched (best overlap) with their segment in `b`;
    labels < 0 are treated as one 'dropped' class."""
    a = np.asarray(a).astype(np.int64)
    b = np.asarray(b).astype(np.int64)
    a = np.where(a < 0, -1, a) + 1
    b = np.where(b < 0, -1, b) + 1
    key = a * (b.max() + 1) + b
    uk, cnt = np.unique(key, return_counts=True)
    ua = uk // (b.max() + 1)
    best = {}
    for x, c in zip(ua, cnt):
        if c > best.get(x, 0):
            best[x] = c
    return sum(best.values()) / len(a)


def p2_protocol(lab_test, lab_ref, point_voxel, used=None, min_voxels=20):
    """SURVEY.md 8c P2, all three clauses, of point labels `lab_test` (the path under test) against `lab_ref` (the oracle in
    the reference's arithmetic), `point_voxel` = node (voxel / supervoxel) of every point (< 0: in none):

    * agreement: share of the used nodes that lie in matching segments after best-match relabelling (every oracle
      segment is matched to the test segment it shares most nodes with; dropped nodes, label < 0, are one class);
    * min_iou:   smallest point-set IoU between an oracle segment of >= `min_voxels` nodes and its best match by points
      (1.0 if there is no such segment); `worst` names that segment;
    * kept_test / kept_ref: kept-segment counts (labels >= 0 present).
    Returns a dict; `assert_p2` applies the stated tolerances."""
    lt = np.asarray(lab_test).astype(np.int64)
    lr = np.asarray(lab_ref).astype(np.int64)
    pv = np.asarray(point_voxel).astype(np.int64)
    assert lt.shape == lr.shape == pv.shape
    ok = pv >= 0
    lt, lr, pv = np.where(lt < 0, -1, lt)[ok] + 1, np.where(lr < 0, -1, lr)[ok] + 1, pv[ok]
    nt, nr = int(lt.max(initial=0)) + 1, int(lr.max(initial=0)) + 1
    # node labels: every point of a node carries the node's label
    V = int(pv.max(initial=-1)) + 1
    vt, vr = np.zeros(V, np.int64), np.zeros(V, np.int64)
    vt[pv], vr[pv] = lt, lr
    assert np.array_equal(vt[pv], lt) and np.array_equal(vr[pv], lr), "a node's points carry different labels"
    present = np.zeros(V, bool)
    present[pv] = True
    sel = present if used is None else (present & np.asarray(used).astype(bool)[:V])
    # clause 1 on nodes
    uk, cnt = np.unique(vr[sel] * nt + vt[sel], return_counts=True)
    best = np.zeros(nr, np.int64)
    np.maximum.at(best, uk // nt, cnt)
    agreement = best.sum() / max(1, int(sel.sum()))
    # clause 2 on points, oracle segments with >= min_voxels nodes
    vox_per_ref = np.bincount(vr[present], minlength=nr)
    big = np.nonzero(vox_per_ref >= min_voxels)[0]
    big = big[big > 0]
    pk, pc = np.unique(lr * nt + lt, return_counts=True)
    size_t, size_r = np.bincount(lt, minlength=nt), np.bincount(lr, minlength=nr)
    inter = np.zeros(nr, np.int64)
    match = np.zeros(nr, np.int64)
    for k, c in zip(pk, pc):
        r, t = divmod(int(k), nt)
        if t > 0 and c > inter[r]:
            inter[r], match[r] = c, t
    min_iou, worst = 1.0, None
    for r in big:
        iou = inter[r] / (size_r[r] + size_t[match[r]] - inter[r]) if inter[r] else 0.0
        if iou < min_iou:
            min_iou, worst = float(iou), dict(ref_label=int(r) - 1, points=int(size_r[r]), nodes=int(vox_per_ref[r]),
                                              match=int(match[r]) - 1, match_points=int(size_t[match[r]]), iou=float(iou))
    return dict(agreement=float(agreement), min_iou=min_iou, worst=worst, big_segments=int(big.size),
                kept_test=int(np.unique(lt[lt > 0]).size), kept_ref=int(np.unique(lr[lr > 0]).size))


def assert_p2(lab_test, lab_ref, point_voxel, used=None, agreement=0.995, iou=0.98, count_tol=0.01):
    """The stated tolerance of SURVEY.md 8c P2: >= 99.5 % of the used nodes in matching segments, point-set IoU >= 0.98 for every
    oracle segment of >= 20 nodes, kept-segment count within +-1 %."""
    r = p2_protocol(lab_test, lab_ref, point_voxel, used)
    assert r["agreement"] >= agreement, r
    assert r["min_iou"] >= iou, r
    assert abs(r["kept_test"] - r["kept_ref"]) <= count_tol * r["kept_ref"], r
    return r


# ---------------------------------------------------------------- per-segment descriptors: numpy float64 reference
SD_CHUNK = 2048   # virtual points per chunk of csrc/segdesc.hip (SD_TB * SD_PPT)


def ref_descriptors(xyz, labels, K):
    """Two-pass mean, centred covariance (1/n), eigh -- float64 over the float32 points labelled 0 .. K-1.  A label that no point carries
    gets n_points 0, the empty box (+inf, -inf) and NaN moments.  zero_signs (K, 6): the segment holds both +0.0 and -0.0 in that box
    entry's coordinate, where include/vgs.h lets a zero bound carry either sign."""
    m = labels >= 0
    lab = labels[m].astype(np.int64)
    x32 = xyz[m, :3]
    x = x32.astype(np.float64)
    n = np.bincount(lab, minlength=K).astype(np.int64)
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.stack([np.bincount(lab, x[:, a], minlength=K) for a in range(3)], axis=1) / n[:, None]
        mean = mean + np.stack([np.bincount(lab, x[:, a] - mean[lab, a], minlength=K) for a in range(3)], axis=1) / n[:, None]
        d = x - mean[lab]
        cov = np.stack([np.bincount(lab, d[:, i] * d[:, j], minlength=K) for i, j in pairs], axis=1) / n[:, None]
    order = np.argsort(lab, kind="stable")
    starts = np.concatenate([[0], np.cumsum(n)[:-1]])
    xs = x32[order]
    has = n > 0
    bbox = np.empty((K, 6), dtype=np.float32)
    bbox[:, :3], bbox[:, 3:] = np.inf, -np.inf
    if has.any():   # (reduceat over an empty run would return the next run's first point)
        bbox[has] = np.concatenate([np.minimum.reduceat(xs, starts[has], axis=0), np.maximum.reduceat(xs, starts[has], axis=0)], axis=1)
    zero = x32 == 0
    pos, neg = zero & ~np.signbit(x32), zero & np.signbit(x32)
    both = np.stack([(np.bincount(lab, pos[:, a], minlength=K) > 0) & (np.bincount(lab, neg[:, a], minlength=K) > 0) for a in range(3)], axis=1)
    M = np.zeros((K, 3, 3))
    for c, (i, j) in enumerate(pairs):
        M[:, i, j] = cov[:, c]
        M[:, j, i] = cov[:, c]
    w = np.full((K, 3), np.nan)
    v = np.full((K, 3, 3), np.nan)
    if has.any():
        w[has], v[has] = np.linalg.eigh(M[has])
    return dict(n_points=n, bbox6=bbox, centroid3=mean, cov6=cov, evals3=w, evecs=v, zero_signs=np.concatenate([both, both], axis=1))


def ref_features(ev, svgs):
    """vm_eigen_features (csrc/vgs_math.h) in float32 numpy, from ascending eigenvalues."""
    ev = ev.astype(np.float32)
    F = np.zeros((ev.shape[0], 8), dtype=np.float32)
    with np.errstate(all="ignore"):
        s = np.sqrt(ev[:, 0] * ev[:, 0] + ev[:, 1] * ev[:, 1] + ev[:, 2] * ev[:, 2])
        e3, e2, e1 = ev[:, 0] / s, ev[:, 1] / s, ev[:, 2] / s
        sm = e1 + e2 + e3
        cur = e3 / sm
        z1 = e1 == 0
        lin = np.where(z1, np.float32(0), (e1 - e2) / e1)
        pla = np.where(z1, np.float32(1), (e2 - e3) / e1)
        sca = np.where(z1, np.float32(0), e3 / e1)
        ani = np.where((z1 if svgs else e2 == 0), np.float32(0), (e1 - e3) / e1)
        prod = e1 * e2 * e3
        ent = np.where(prod == 0, np.float32(0), -1.0 * (e1 * np.log(e1) + e2 * np.log(e2) + e3 * np.log(e3)))
        omn = np.where(prod == 0, np.float32(0), np.exp(np.log(prod) * np.float32(0.33333334)))
    cols = [lin, pla, sca, ani, cur] if svgs else [lin, pla, sca, cur, ani]
    F[:] = np.stack(cols + [ent, sm, omn], axis=1).astype(np.float32)
    F[(ev == 0).all(axis=1)] = 0
    return F


def same_box(got, ref, zero_signs):
    """Box entries equal bit for bit, except a zero bound in a coordinate where the segment holds both +0.0 and -0.0 (zero_signs of
    ref_descriptors): include/vgs.h lets it carry either sign, so it compares by value."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    if got.shape != ref.shape:
        return False
    return bool(((got.view(np.uint32) == ref.view(np.uint32)) | (zero_signs & (got == 0) & (ref == 0))).all())


def check_descriptors(eng, xyz, svgs):
    K = eng.counts()["kept"]
    got = eng.segment_descriptors()
    labels = eng.point_labels()
    assert K > 0 and labels.max() == K - 1
    ref = ref_descriptors(xyz, labels, K)
    assert np.array_equal(got["n_points"], ref["n_points"])
    _, kept = eng.node_labels()
    assert np.array_equal(got["n_nodes"], np.bincount(kept[kept >= 0], minlength=K).astype(np.int32))
    assert same_box(got["bbox6"], ref["bbox6"], ref["zero_signs"])
    c = got["centroid3"]
    assert (np.abs(c - ref["centroid3"]) <= 1e-9 * (1 + np.linalg.norm(ref["centroid3"], axis=1))[:, None]).all()
    tr = ref["cov6"][:, [0, 3, 5]].sum(axis=1)
    assert (np.abs(got["cov6"] - ref["cov6"]) <= 1e-8 * tr[:, None] + 1e-30).all()
    lmax = ref["evals3"][:, 2]
    assert (got["evals3"] >= 0).all() and (np.diff(got["evals3"], axis=1) >= 0).all()
    assert (np.abs(got["evals3"] - np.maximum(ref["evals3"], 0)) <= 1e-8 * lmax[:, None] + 1e-30).all()
    V = got["evecs9"].reshape(K, 3, 3)   # [k, r, j] = component r of eigenvector j
    assert np.allclose(np.einsum("kri,krj->kij", V, V), np.eye(3)[None], atol=1e-10)
    for j in range(3):
        col = V[:, :, j]
        big = col[np.arange(K), np.argmax(np.abs(col), axis=1)]   # argmax: the lowest index on a tie
        assert (big > 0).all(), j
        w = ref["evals3"]
        gap = np.minimum(np.abs(w[:, j] - w[:, j - 1]) if j > 0 else np.inf, np.abs(w[:, j + 1] - w[:, j]) if j < 2 else np.inf)
        sel = gap >= 1e-3 * lmax
        dots = np.abs((col * ref["evecs"][:, :, j]).sum(axis=1))
        assert (dots[sel] >= 1 - 1e-6).all(), (j, dots[sel].min())
    one = got["n_points"] == 1
    assert (got["cov6"][one] == 0).all() and (got["eigen8"][one] == 0).all()
    assert (V[one] == np.eye(3)[None]).all()
    np.testing.assert_allclose(got["eigen8"], ref_features(got["evals3"], svgs), rtol=1e-5, atol=1e-6)
    return got


# ---------------------------------------------------------------- segment adjacency graph: numpy ground truth
def graph_truth(lab, off, idx, K, weight=None, sample=None, seed=0):
    """The segment graph by its definition (include/vgs.h), independent of any engine.  lab: effective label of every node (-1: takes no
    part); (off, idx): the stored adjacency rows as CSR; K: kept segments; weight(u, v) -> float32 w(u, v) for arrays of node ids u < v
    (None: counts only).  sample: weights of that many seeded edges, or of the given edge rows (returned as 'wsel'); None: of every edge.
    Also returned: 'key' (the sort key min(a, b) * K + max(a, b) of every edge) and 'row_labels' (distinct boundary labels per row)."""
    lab = np.asarray(lab).astype(np.int64)
    off = np.asarray(off).astype(np.int64)
    V = lab.shape[0]
    assert lab.max(initial=-1) < K
    u = np.repeat(np.arange(V, dtype=np.int64), np.diff(off))
    v = np.asarray(idx).astype(np.int64)
    m = (lab[u] >= 0) & (lab[v] >= 0) & (lab[u] != lab[v])
    u, v = u[m], v[m]
    # the predicate is symmetric: every directed pair appears both ways
    assert np.array_equal(np.unique(u * V + v), np.unique(v * V + u))
    la, lb = lab[u], lab[v]
    key = np.minimum(la, lb) * K + np.maximum(la, lb)
    keys = np.unique(key)
    E = keys.shape[0]
    eid = np.searchsorted(keys, key)
    lt = u < v
    Kd = max(int(K), 1)
    out = dict(seg_ab=np.stack([keys // Kd, keys % Kd], axis=1).astype(np.int32).reshape(E, 2),
               n_pairs=np.bincount(eid[lt], minlength=E).astype(np.int64))
    nk = np.unique(u * K + lb)
    nu, nb = nk // Kd, nk % Kd
    na_ = lab[nu]
    e2 = np.searchsorted(keys, np.minimum(na_, nb) * K + np.maximum(na_, nb))
    side_a = na_ < nb
    out["nodes_ab"] = np.stack([np.bincount(e2[side_a], minlength=E), np.bincount(e2[~side_a], minlength=E)], axis=1).astype(np.int32).reshape(E, 2)
    out["key"] = keys
    out["row_labels"] = np.bincount(nu, minlength=V)
    if weight is None:
        return out
    if sample is None:
        wsel = np.arange(E)
    elif np.ndim(sample) == 0:
        wsel = np.arange(E) if sample >= E else np.sort(np.random.default_rng(seed).choice(E, size=int(sample), replace=False))
    else:
        wsel = np.unique(np.asarray(sample, dtype=np.int64))
    take = lt & np.isin(eid, wsel)
    w = np.asarray(weight(u[take], v[take]), dtype=np.float32)
    ei = eid[take]
    fin = ~np.isnan(w)
    out["n_finite"] = np.bincount(ei[fin], minlength=E).astype(np.int64)
    out["w_sum"] = np.bincount(ei[fin], weights=w[fin].astype(np.float64), minlength=E)
    mn = np.full(E, np.inf, dtype=np.float32)
    mx = np.full(E, -np.inf, dtype=np.float32)
    np.minimum.at(mn, ei[fin], w[fin])
    np.maximum.at(mx, ei[fin], w[fin])
    none = out["n_finite"] == 0
    mn[none] = np.nan
    mx[none] = np.nan
    out["w_min"], out["w_max"] = mn, mx
    out["wsel"] = wsel
    return out


def graph_inputs(eng):
    """(effective labels, row offsets, row ids, K) of an engine: a used node keeps its kept label, every other node gets -1."""
    off, idx = eng.lists("adjacency")
    _, kept = eng.node_labels()
    used = eng.attributes()["used"].astype(bool)
    return np.where(used, kept, -1).astype(np.int64), off, idx, eng.counts()["kept"]


def pair_weights(eng, u, v):
    """w(u, v) for u < v from Engine.local_weights(u): the entry of the ordered pair (u first) of u's own local graph."""
    w = np.empty(u.shape[0], dtype=np.float32)
    order = np.argsort(u, kind="stable")
    us, starts = np.unique(u[order], return_index=True)
    ends = np.append(starts[1:], order.shape[0])
    for node, s, e in zip(us.tolist(), starts.tolist(), ends.tolist()):
        ids, W = eng.local_weights(node)
        srt = np.argsort(ids)
        sel = order[s:e]
        pv = srt[np.searchsorted(ids[srt], v[sel])]
        assert np.array_equal(ids[pv], v[sel])
        pu = int(np.nonzero(ids == node)[0][0])
        w[sel] = W[pu, pv]
    return w


def ref_graph(eng, sample=None, seed=0):
    """The table by definition (graph_truth) over the engine's own rows, node labels and local-cut weights."""
    lab, off, idx, K = graph_inputs(eng)
    return graph_truth(lab, off, idx, K, lambda a, b: pair_weights(eng, a, b), sample=sample, seed=seed)


def check_graph(eng, sample=None, ref=None):
    got = eng.segment_graph()
    if ref is None:
        ref = ref_graph(eng, sample=sample)
    E = ref["seg_ab"].shape[0]
    assert got["seg_ab"].shape == (E, 2)
    for k in ("seg_ab", "n_pairs", "nodes_ab"):
        assert np.array_equal(got[k], ref[k]), k
    s = ref["wsel"]
    assert np.array_equal(got["n_finite"][s], ref["n_finite"][s])
    assert np.array_equal(got["w_min"][s].view(np.uint32), ref["w_min"][s].view(np.uint32))
    assert np.array_equal(got["w_max"][s].view(np.uint32), ref["w_max"][s].view(np.uint32))
    rs, gs = ref["w_sum"][s], got["w_sum"][s]
    assert (np.abs(gs - rs) <= 1e-10 * np.abs(rs) + 1e-300).all()
    # invariants of the definition
    a, b = got["seg_ab"][:, 0], got["seg_ab"][:, 1]
    assert (a < b).all() and (a >= 0).all() and (b < eng.counts()["kept"]).all()
    assert (np.diff(a.astype(np.int64) * (1 << 32) + b) > 0).all()   # ascending (a, b), each edge once
    na, nb = got["nodes_ab"][:, 0].astype(np.int64), got["nodes_ab"][:, 1].astype(np.int64)
    assert (np.maximum(na, nb) <= got["n_pairs"]).all() and (got["n_pairs"] <= na * nb).all()
    assert (got["n_finite"] <= got["n_pairs"]).all()
    return got


# ---------------------------------------------------------------- which structural limits of the two tables a scene reaches
def segment_limits(K, point_labels, node_label=None, node_points=None, truth=None, graph=None):
    """The limits of csrc/segdesc.hip and csrc/seggraph.hip that a scene reaches, from numpy alone:
      K; seg_points and seg_mod (every segment's points, and those modulo SD_CHUNK);
      with node_label / node_points (kept label and points of every node; a segment's nodes in ascending id, the descriptor's order):
      max_node_points, first_node_chunks (most chunks a segment's first node covers), nodes_on_chunk_start (nodes other than a segment's
      first whose first point starts a chunk);
      with truth (graph_truth's dict): max_key (the largest sort key min(a, b) * K + max(a, b)), max_row_labels (most distinct boundary
      labels in one row), max_edge_records (most records of one edge = nodes_ab[0] + nodes_ab[1]);
      with graph (a table with n_pairs / n_finite): nan_edges (0 < n_finite < n_pairs) and no_finite_edges (n_finite == 0)."""
    pl = np.asarray(point_labels)
    seg = np.bincount(pl[pl >= 0], minlength=K).astype(np.int64)
    out = dict(K=int(K), seg_points=seg, seg_mod=seg % SD_CHUNK)
    if node_label is not None:
        nl = np.asarray(node_label).astype(np.int64)
        npt = np.asarray(node_points).astype(np.int64)
        sel = np.nonzero(nl >= 0)[0]
        order = sel[np.argsort(nl[sel], kind="stable")]   # segments in label order, each one's nodes ascending
        lab_s, pts_s = nl[order], npt[order]
        first = np.ones(order.shape[0], dtype=bool)
        first[1:] = lab_s[1:] != lab_s[:-1]
        vp = np.concatenate([[0], np.cumsum(pts_s)[:-1]]).astype(np.int64)
        at = vp - np.maximum.accumulate(np.where(first, vp, 0))   # the node's first point inside its segment
        out["max_node_points"] = int(pts_s.max(initial=0))
        out["first_node_chunks"] = int(((pts_s[first] + SD_CHUNK - 1) // SD_CHUNK).max(initial=0))
        out["nodes_on_chunk_start"] = int((~first & (at % SD_CHUNK == 0)).sum())
    if truth is not None:
        out["max_key"] = int(truth["key"].max(initial=0))
        out["max_row_labels"] = int(truth["row_labels"].max(initial=0))
        out["max_edge_records"] = int(truth["nodes_ab"].astype(np.int64).sum(axis=1).max(initial=0))
    if graph is not None:
        out["nan_edges"] = int(((graph["n_finite"] > 0) & (graph["n_finite"] < graph["n_pairs"])).sum())
        out["no_finite_edges"] = int((graph["n_finite"] == 0).sum())
    return out


def engine_limits(eng, truth=None, graph=None):
    """segment_limits of an engine's segmentation (nodes: its voxels or supervoxels, their points from the point-to-node map)."""
    _, kept = eng.node_labels()
    pv = eng.point_voxel()
    npts = np.bincount(pv[pv >= 0], minlength=kept.shape[0])
    return segment_limits(eng.counts()["kept"], eng.point_labels(), kept, npts, truth=truth, graph=graph)


def canonical_labels(lab):
    """Relabel so that equal partitions give equal arrays: label = smallest member index of the class."""
    lab = np.asarray(lab)
    out = np.full(lab.shape, -1, dtype=np.int64)
    valid = lab >= 0
    if valid.any():
        idx = np.arange(lab.size)
        first = np.full(lab.max() + 1, lab.size, dtype=np.int64)
        np.minimum.at(first, lab[valid], idx[valid])
        out[valid] = first[lab[valid]]
    return out


# ---------------------------------------------------------------- everything a caller can read after run(), byte for byte
# Schedule counters (Engine.schedule_counters) that are left out of a snapshot, each with the reason.  A counter belongs here only if two
# FRESH engines on the same cloud and parameters report different values for it, i.e. if it depends on timing, not on state.
# Measured on an MI355X: four fresh engines on sequence_frames' frame A (town_scene(20000), default parameters) and two on every other
# frame agreed on all thirteen counters (and on every other key of the snapshot), so none is left out;
# test_gpu_sequence.test_fresh_engines_agree_with_the_oracle_and_each_other repeats the comparison of two fresh engines on A in every run.
SNAPSHOT_TIMING_COUNTERS = {}

SNAPSHOT_LISTS = ("adjacency", "connect_cut", "connect_cross", "connect_final")
SNAPSHOT_CLASSES = 7


def snapshot_inputs(n):
    """The caller-supplied attributes of a snapshot for a cloud of n points: a seeded 3-channel float field with some NaN and an inf, and
    seeded classes of which some lie outside 0 .. SNAPSHOT_CLASSES - 1."""
    rng = np.random.default_rng(1000 + n)
    field = (rng.standard_normal((n, 3)) * np.array([1.0, 50.0, 1e-3]) + np.array([0.0, 1.0e4, 0.0])).astype(np.float32)
    field[rng.random(n) < 0.03, 1] = np.nan
    field[rng.random(n) < 0.01, 2] = np.inf
    classes = rng.integers(-1, SNAPSHOT_CLASSES + 1, size=n).astype(np.int32)
    return field, classes


def snapshot(eng):
    """Everything a caller can read from a segmented Engine, as a flat dict of numpy arrays: counts (no times), bbox, voxel table, point ->
    voxel map, voxel centres, attributes, adjacency counts, the four ragged lists and the cluster lists in both element orders, node and
    point labels, segment descriptors, oriented boxes in both frames, segment graph, the field statistics and class histogram of
    snapshot_inputs, and the schedule counters except SNAPSHOT_TIMING_COUNTERS.  Compare two of them with assert_same_snapshot."""
    out = {}

    def put(prefix, d):
        for k, v in d.items():
            out[prefix + "." + k] = np.asarray(v)

    c = eng.counts()
    out["counts"] = np.array([c[k] for k in sorted(c)], dtype=np.int64)
    out["counts.names"] = np.array(sorted(c))
    out["bbox"] = eng.bbox()
    put("voxel_table", eng.voxel_table())
    out["point_voxel"] = eng.point_voxel()
    out["voxel_centers"] = eng.voxel_centers()
    put("attributes", eng.attributes())
    out["adjacency_counts"] = eng.adjacency_counts()
    for which in SNAPSHOT_LISTS:
        for order in ("voxel_id", "reference"):
            off, idx = eng.lists(which, order)
            out[f"lists.{which}.{order}.offsets"], out[f"lists.{which}.{order}.ids"] = off, idx
    out["node_labels.root"], out["node_labels.kept"] = eng.node_labels()
    out["point_labels"] = eng.point_labels()
    for order in ("voxel_id", "reference"):
        off, idx = eng.clusters(order)
        out[f"clusters.{order}.offsets"], out[f"clusters.{order}.ids"] = off, idx
    put("segment_descriptors", eng.segment_descriptors())
    for frame in ("principal", "upright"):
        put("segment_boxes." + frame, eng.segment_boxes(frame))
    put("segment_graph", eng.segment_graph())
    field, classes = snapshot_inputs(eng.n)
    put("segment_field_stats", eng.segment_field_stats(field))
    put("segment_class_histogram", eng.segment_class_histogram(classes, SNAPSHOT_CLASSES))
    sc = eng.schedule_counters()
    names = [k for k in sc if k not in SNAPSHOT_TIMING_COUNTERS]
    out["schedule_counters"] = np.array([sc[k] for k in names], dtype=np.int64)
    out["schedule_counters.names"] = np.array(names)
    return out


def snapshot_diff(a, b):
    """Keys whose arrays differ in dtype, shape or raw bytes (NaN payloads and signed zeros included)."""
    bad = [k for k in sorted(set(a) | set(b)) if k not in a or k not in b]
    for k in sorted(set(a) & set(b)):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(k)
    return bad


def assert_same_snapshot(got, want, what=""):
    bad = snapshot_diff(got, want)
    assert not bad, f"{what}: {len(bad)} of {len(want)} results differ from the fresh engine's: {bad}"
