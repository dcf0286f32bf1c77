"""The adjacency graph of a per-point labelling by its definition (include/vgs.h, vgs_point_label_graph), in plain numpy: no engine, no
shared code.  Inputs: the labels, the node of every point (Engine.point_voxel()), the rows of every node as CSR (Engine.lists("adjacency")),
the used flag of every node, K and weight(u, v) -> float32 for arrays of node ids u < v (both used).  Contacts come from the symmetric
closure of the rows."""
import numpy as np

FIELDS = ("seg_ab", "n_shared", "n_pairs", "n_finite", "nodes_ab", "w_sum", "w_min", "w_max")


def _cross(first_a, count_a, first_b, count_b):
    """for every row i the index pairs (first_a[i] + p, first_b[i] + q), p < count_a[i], q < count_b[i]; also the row of every pair"""
    tot = count_a * count_b
    row = np.repeat(np.arange(tot.shape[0]), tot)
    k = np.arange(row.shape[0]) - np.repeat(np.cumsum(tot) - tot, tot)
    cb = count_b[row]
    return row, first_a[row] + k // np.maximum(cb, 1), first_b[row] + k % np.maximum(cb, 1)


def label_graph(labels, point_voxel, off, idx, used, K, weight=None):
    labels = np.asarray(labels).astype(np.int64)
    pv = np.asarray(point_voxel).astype(np.int64)
    off = np.asarray(off).astype(np.int64)
    idx = np.asarray(idx).astype(np.int64)
    used = np.asarray(used).astype(bool)
    V = off.shape[0] - 1
    K = int(K)
    assert labels.max(initial=-1) < max(K, 0) or (labels < 0).all()
    lab = labels >= 0
    n_skipped = int((lab & (pv < 0)).sum())
    Kd = max(K, 1)
    # vertices, by node then label
    vk = np.unique(pv[lab & (pv >= 0)] * Kd + labels[lab & (pv >= 0)])
    vnode, vlab = vk // Kd, vk % Kd
    nfirst = np.searchsorted(vnode, np.arange(V))
    ncount = np.searchsorted(vnode, np.arange(V), side="right") - nfirst
    # adjacent node pairs v < w: the symmetric closure of the rows
    u = np.repeat(np.arange(V, dtype=np.int64), np.diff(off))
    m = u != idx
    pk = np.unique(np.minimum(u[m], idx[m]) * max(V, 1) + np.maximum(u[m], idx[m]))
    pa, pb = pk // max(V, 1), pk % max(V, 1)
    keep = (ncount[pa] > 0) & (ncount[pb] > 0)
    pa, pb = pa[keep], pb[keep]
    # contacts: every (label of v, label of w) with different labels
    row, ia, ib = _cross(nfirst[pa], ncount[pa], nfirst[pb], ncount[pb])
    la, lb = vlab[ia], vlab[ib]
    d = la != lb
    row, ia, ib, la, lb = row[d], ia[d], ib[d], la[d], lb[d]
    ckey = np.minimum(la, lb) * Kd + np.maximum(la, lb)
    # shared nodes: every pair of labels a < b of one node
    many = np.nonzero(ncount > 1)[0]
    _, sa, sb = _cross(nfirst[many], ncount[many], nfirst[many], ncount[many])
    s = vlab[sa] < vlab[sb]
    skey = vlab[sa][s] * Kd + vlab[sb][s]
    keys = np.unique(np.concatenate([ckey, skey]))
    E = keys.shape[0]
    ce, se = np.searchsorted(keys, ckey), np.searchsorted(keys, skey)
    out = dict(seg_ab=np.stack([keys // Kd, keys % Kd], axis=1).astype(np.int32).reshape(E, 2),
               n_shared=np.bincount(se, minlength=E).astype(np.int64), n_pairs=np.bincount(ce, minlength=E).astype(np.int64))
    # the vertices in a contact, per edge and side
    nv = max(vk.shape[0], 1)
    side_a = np.unique(ce * nv + np.where(la < lb, ia, ib))
    side_b = np.unique(ce * nv + np.where(la < lb, ib, ia))
    out["nodes_ab"] = np.stack([np.bincount(side_a // nv, minlength=E), np.bincount(side_b // nv, minlength=E)], axis=1).astype(np.int32).reshape(E, 2)
    out["n_edges"], out["n_skipped"] = E, n_skipped
    if weight is None:
        return out
    # weights: of the contacts between two used nodes, the lower node id first
    both = used[pa] & used[pb]
    wp = np.full(pa.shape[0], np.nan, dtype=np.float32)
    need = np.zeros(pa.shape[0], dtype=bool)
    need[row] = True
    need &= both
    if need.any():
        wp[need] = np.asarray(weight(pa[need], pb[need]), dtype=np.float32)
    w = wp[row]
    fin = both[row] & ~np.isnan(w)
    out["n_finite"] = np.bincount(ce[fin], minlength=E).astype(np.int64)
    out["w_sum"] = np.bincount(ce[fin], weights=w[fin].astype(np.float64), minlength=E).astype(np.float64)
    mn = np.full(E, np.inf, dtype=np.float32)
    mx = np.full(E, -np.inf, dtype=np.float32)
    np.minimum.at(mn, ce[fin], w[fin])
    np.maximum.at(mx, ce[fin], w[fin])
    none = out["n_finite"] == 0
    mn[none] = np.nan
    mx[none] = np.nan
    out["w_min"], out["w_max"] = mn, mx
    return out


def diff(got, ref, w_sum_rtol=1e-10):
    """the fields in which two tables differ ([] = none): integers and extrema exactly (the floats as bit patterns), w_sum within
    |got - ref| <= w_sum_rtol * |ref|"""
    bad = []
    for k in ("n_edges", "n_skipped"):
        if k in ref and int(got[k]) != int(ref[k]):
            bad.append(k)
    for k in FIELDS:
        if k not in ref:
            continue
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        if g.shape != r.shape:
            bad.append(k)
        elif k == "w_sum":
            if not (np.abs(g - r) <= w_sum_rtol * np.abs(r) + 1e-300).all():
                bad.append(k)
        elif k in ("w_min", "w_max"):
            if g.astype(np.float32).view(np.uint32).tobytes() != r.astype(np.float32).view(np.uint32).tobytes():
                bad.append(k)
        elif not np.array_equal(g, r):
            bad.append(k)
    return bad
