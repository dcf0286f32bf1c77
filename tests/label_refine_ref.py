"""numpy float32 restatement of the point-level label refinement (include/vgs.h, vgs_refine_point_labels): brute force over every point
and every candidate of its node, no interior shortcut.  numpy's separate multiply and add and its correctly rounded sqrt reproduce the
expressions of vm_refine_cost (csrc/vgs_math.h) to the bit, so the engine's labels are compared with `==`.

Inputs, as the engine's or the oracle's getters hand them out: the points, point_voxel (N, -1 = in no node), the attributes dict
(centroid, normal, used), the kept node labels (V) and lists("adjacency") as (offsets, ids)."""
import numpy as np

F = np.float32


def _max(a, b):
    """vm_max: a where a > b, else b (b when a is NaN)"""
    return np.where(a > b, a, b)


def refine_cost(p, c, n, patch_radius):
    """cost of the candidates (c, n: (m, 3)) for the points p (k, 3): (k, m) float32"""
    r = F(patch_radius)
    with np.errstate(all="ignore"):
        d0 = p[:, None, 0] - c[None, :, 0]
        d1 = p[:, None, 1] - c[None, :, 1]
        d2 = p[:, None, 2] - c[None, :, 2]
        h = (n[None, :, 0] * d0 + n[None, :, 1] * d1) + n[None, :, 2] * d2
        q = (d0 * d0 + d1 * d1) + d2 * d2
        t = np.sqrt(_max(q - h * h, F(0)))
        e = _max(t - r, F(0))
        cost = h * h + e * e
    assert cost.dtype == np.float32
    return cost


def node_state(attr, kept):
    """A per node (the kept label of a used node, -1 otherwise) and which nodes can be candidates"""
    used = np.asarray(attr["used"]) != 0
    kept = np.asarray(kept, dtype=np.int32)
    A = np.where(used, kept, -1).astype(np.int32)
    pos = (attr["centroid"] != 0).all(axis=1)   # VGS_F_POS
    nrm = (attr["normal"] != 0).all(axis=1)     # VGS_F_NRM
    cand = used & (kept >= 0) & pos & nrm
    return A, cand


def candidates_of(v, off, idx, cand):
    w = np.unique(np.concatenate([[v], idx[off[v]:off[v + 1]]]).astype(np.int64))   # ascending ids
    return w[cand[w]]


def working_nodes(attr, kept, adjacency, fill=True):
    """bool per node: a labelled node with a candidate of another label, or (fill) an unlabelled node with a candidate"""
    off, idx = adjacency
    A, cand = node_state(attr, kept)
    out = np.zeros(A.shape[0], dtype=bool)
    for v in range(A.shape[0]):
        w = candidates_of(v, off, idx, cand)
        if A[v] >= 0:
            out[v] = bool((kept[w] != A[v]).any())
        else:
            out[v] = bool(fill) and w.size > 0
    return out


def refine_labels(xyz, point_voxel, attr, kept, adjacency, patch_radius, switch_ratio=0.25, fill=True):
    """(refined labels (N) int32, counts dict) by the rule of include/vgs.h"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)[:, :3]
    off, idx = adjacency
    kept = np.asarray(kept, dtype=np.int32)
    A, cand = node_state(attr, kept)
    cen = np.ascontiguousarray(attr["centroid"], dtype=np.float32)
    nrm = np.ascontiguousarray(attr["normal"], dtype=np.float32)
    pv = np.asarray(point_voxel, dtype=np.int64)
    finite = np.isfinite(xyz).all(axis=1)
    inside = (pv >= 0) & finite
    out = np.full(xyz.shape[0], -1, dtype=np.int32)
    out[inside] = A[pv[inside]]
    before = out.copy()
    sr = F(switch_ratio)
    order = np.argsort(pv, kind="stable")
    order = order[inside[order]]
    bounds = np.flatnonzero(np.diff(pv[order])) + 1
    for pts in np.split(order, bounds):
        if pts.size == 0:
            continue
        v = int(pv[pts[0]])
        if A[v] < 0 and not fill:
            continue
        w = candidates_of(v, off, idx, cand)
        if w.size == 0:
            continue
        cost = refine_cost(xyz[pts], cen[w], nrm[w], patch_radius)
        cost = np.where(np.isfinite(cost), cost, F(np.inf))          # a non-finite cost: no candidate for that point
        b = np.argmin(cost, axis=1)                                  # the first minimum: the smallest id (w ascends)
        cb = cost[np.arange(pts.size), b]
        has = np.isfinite(cb)
        lab_b = kept[w[b]]
        if A[v] >= 0:
            own = kept[w] == A[v]
            if not own.any():
                continue
            c_own = cost[:, own].min(axis=1)
            with np.errstate(all="ignore"):
                take = np.isfinite(c_own) & (cb < sr * c_own)
            out[pts] = np.where(take, lab_b, A[v])
        else:
            out[pts] = np.where(has, lab_b, -1)
    work = working_nodes(attr, kept, adjacency, fill)
    counts = dict(working_nodes=int(work.sum()), points_examined=int(work[pv[inside]].sum()),
                  points_changed=int(((before >= 0) & (out != before)).sum()), points_filled=int(((before < 0) & (out >= 0)).sum()))
    return out, counts


def majority_errors(labels, truth):
    """points whose truth is not the majority truth of their segment (label >= 0), plus nothing for label -1"""
    labels = np.asarray(labels)
    truth = np.asarray(truth)
    m = labels >= 0
    K = int(labels.max()) + 1 if m.any() else 0
    T = int(truth.max()) + 1
    tab = np.zeros((K, T), dtype=np.int64)
    np.add.at(tab, (labels[m], truth[m]), 1)
    return int(tab.sum() - tab.max(axis=1).sum()) if K else 0


def floor_and_wall(seed=1, n=60_000):
    """the floor-and-wall scene of DESIGN.md section 8 and its truth (0 floor, 1 wall).  Each surface is one (n, 3) block of uniforms --
    column k for coordinate k -- followed by n normals for the coordinate across the surface; this order of the draws reproduces the counts
    recorded where the rule was proposed (557 mislabelled and 1 696 dropped points at voxel_size 0.25)."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, 3))
    floor = np.stack([4 * u[:, 0] + 0.013, 4 * u[:, 1] + 0.007, rng.normal(0, 0.005, n) + 0.011], axis=1)
    u = rng.random((n, 3))
    wall = np.stack([rng.normal(0, 0.005, n) + 0.013, 4 * u[:, 1] + 0.007, 3 * u[:, 2] + 0.011], axis=1)
    xyz = np.concatenate([floor, wall]).astype(np.float32)
    truth = np.concatenate([np.zeros(n, np.int32), np.ones(n, np.int32)])
    return xyz, truth
