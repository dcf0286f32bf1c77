"""Plain numpy restatement of the connected parts of a per-point labelling (include/vgs.h, vgs_point_label_components), the reference of
tests/test_gpu_label_components.py.

Vertices are the distinct pairs (label, node) with a point; (l, v) and (l, w) are joined when w is in the adjacency row of v OR v is in
the row of w; a part is a connected component; parts are numbered in ascending (label, smallest node id of the part).  A Python
union-find over the symmetric closure of the rows, nothing clever."""
import numpy as np

FIELDS = ("part_of_point", "part_label", "part_points", "part_nodes", "part_first_node", "label_first", "label_largest")


def label_components(labels, node_of_point, offsets, idx, K):
    """labels, node_of_point: one int per point (negative: no label / no node).  offsets, idx: the rows of Engine.lists(0).  Returns the
    dict of Engine.label_components(labels, K): the seven tables, n_parts and n_skipped."""
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    node = np.asarray(node_of_point).astype(np.int64).reshape(-1)
    offsets = np.asarray(offsets).astype(np.int64).reshape(-1)
    idx = np.asarray(idx).astype(np.int64).reshape(-1)
    K = int(K)
    n = labels.size
    assert node.size == n
    assert not ((labels >= K) & (labels >= 0)).any(), "a label must be negative or below K"
    n_nodes = offsets.size - 1
    skipped = int(((labels >= 0) & (node < 0)).sum())
    live = (labels >= 0) & (node >= 0)
    # vertices in (label, node) order
    code = labels[live] * max(n_nodes, 1) + node[live]
    vcode, inv, vpoints = np.unique(code, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    vlabel, vnode = vcode // max(n_nodes, 1), vcode % max(n_nodes, 1)
    nv = vcode.size
    # every row entry of every vertex's node, as (vertex, code of the vertex it names); then the entries that name a vertex
    rlen = (offsets[vnode + 1] - offsets[vnode]) if nv else np.zeros(0, np.int64)
    src = np.repeat(np.arange(nv, dtype=np.int64), rlen)
    start = np.repeat(offsets[vnode] if nv else np.zeros(0, np.int64), rlen)
    within = np.arange(src.size, dtype=np.int64) - np.repeat(np.cumsum(rlen) - rlen, rlen)
    want = vlabel[src] * max(n_nodes, 1) + idx[start + within]
    at = np.searchsorted(vcode, want)
    hit = (at < nv) & (vcode[np.minimum(at, max(nv - 1, 0))] == want) if nv else np.zeros(0, bool)
    a, b = src[hit], at[hit]
    # the symmetric closure: an entry in either row is the undirected edge
    edges = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1)[a != b], axis=0)
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in edges.tolist():
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    root = np.array([find(i) for i in range(nv)], dtype=np.int64)
    # the root is the smallest vertex of its component: ascending roots = ascending (label, smallest node)
    roots = np.flatnonzero(root == np.arange(nv))
    part_of_root = np.full(nv + 1, -1, np.int64)
    part_of_root[roots] = np.arange(roots.size)
    vpart = part_of_root[root] if nv else np.zeros(0, np.int64)
    C = roots.size
    out = {
        "part_of_point": np.full(n, -1, np.int32),
        "part_label": vlabel[roots].astype(np.int32),
        "part_points": np.bincount(vpart, weights=vpoints, minlength=C).astype(np.int64) if C else np.zeros(0, np.int64),
        "part_nodes": np.bincount(vpart, minlength=C).astype(np.int32) if C else np.zeros(0, np.int32),
        "part_first_node": vnode[roots].astype(np.int32),
    }
    out["part_of_point"][live] = vpart[inv].astype(np.int32)
    out["label_first"] = np.searchsorted(out["part_label"], np.arange(K + 1), side="left").astype(np.int64)
    largest = np.full(K, -1, np.int32)
    for p in range(C - 1, -1, -1):   # descending ids: an equal count of a lower id wins
        l = int(out["part_label"][p])
        if largest[l] < 0 or out["part_points"][p] >= out["part_points"][largest[l]]:
            largest[l] = p
    out["label_largest"] = largest
    out["n_parts"] = int(C)
    out["n_skipped"] = skipped
    return out


def same(a, b):
    """the names of the tables of two results that differ in dtype, shape or bytes (and of the two counts)"""
    bad = [n for n in FIELDS if not (a[n].dtype == b[n].dtype and a[n].shape == b[n].shape and a[n].tobytes() == b[n].tobytes())]
    return bad + [n for n in ("n_parts", "n_skipped") if int(a[n]) != int(b[n])]
