"""Stages a8-a11 of the merge stage, restated sequentially in plain Python from the header of csrc/merge.hip and the reference's steps named
there (crossValidation VS:2111-2179, closestCheck VS:2181-2303, clusteringVoxels VS:2032-2099, the cluster filter VS:963-1009) -- one voxel
after the other, lists mutated in place, nothing of the kernels' data-parallel form:

  crossValidation   for i ascending: a list longer than one keeps the entries whose own list (as it is at that moment) holds i
  closestCheck      for i ascending: a list of exactly one entry whose adjacency vector [count, neighbours ...] is longer than
                    adjacency_min scans that vector in order -- entry 0 is the COUNT read as a voxel id when q7_count_as_index is set
                    (skipped when no voxel has that id) -- and among the entries whose list is longer than one at that moment takes the
                    last one whose weight is >= the best so far (starting from 0; a NaN is never >=); both lists get the other voxel
  clustering        for i ascending: an unclustered voxel collects everything its list reaches, transitively; it is the smallest id
  cluster filter    clusters of more than voxels_min voxels are numbered in the order found; their voxels' points carry the number

Inputs are per voxel: `used`, the adjacency lists of ALL neighbours in scan order, the local cuts' connect lists, and a weight function
(candidate first); see oracle_weight for the one the tests use."""
import numpy as np


def oracle_weight(oracle, nodes, params):
    """w(i, t) = oracle.pair_weight of the 16-float node records, i's first; `nodes`: dict of centroid, normal, eigen, used."""
    rec = {}

    def node(v):
        if v not in rec:
            u = bool(nodes["used"][v])
            rec[v] = oracle.node16(nodes["centroid"][v], nodes["normal"][v], nodes["eigen"][v] if u else None, used=u)
        return rec[v]

    return lambda i, t: np.float32(oracle.pair_weight(node(i), node(t), params))


def merge_stage(used, adjacency, connect_cut, weight, adjacency_min, q7_count_as_index, voxels_min, point_voxel):
    V = len(adjacency)
    used = np.asarray(used).astype(bool)
    # crossValidation
    L = [list(r) for r in connect_cut]
    member = [set(r) for r in L]
    for i in range(V):
        if len(L[i]) > 1:
            L[i] = [s for s in L[i] if i in member[s]]
            member[i] = set(L[i])
    cross = [list(r) for r in L]
    # closestCheck
    attach = np.full(V, -1, dtype=np.int64)
    candidates, eligible, out_of_range = [], {}, 0
    for i in range(V):
        if len(L[i]) != 1:
            continue
        adj = adjacency[i]
        if not len(adj) + 1 > adjacency_min:
            continue
        candidates.append(i)
        best, target, seen = np.float32(0.0), -1, []
        for j in range(len(adj) + 1):
            if j == 0:
                if not q7_count_as_index:
                    continue
                t = len(adj)
                if t >= V:
                    out_of_range += 1
                    continue
            else:
                t = adj[j - 1]
            if len(L[t]) > 1:
                w = weight(i, t)
                seen.append((j, t, w))
                if w >= best:
                    best, target = w, t
        eligible[i] = seen
        if target >= 0:
            attach[i] = target
            L[i].append(target)
            L[target].append(i)
    # clustering
    root = np.full(V, -1, dtype=np.int64)
    for i in range(V):
        if root[i] >= 0:
            continue
        root[i] = i
        stack = [i]
        while stack:
            for v in L[stack.pop()]:
                if root[v] < 0:
                    root[v] = i
                    stack.append(v)
    size = np.bincount(root, minlength=V)
    is_root = root == np.arange(V)
    # cluster filter and labels
    keep = is_root & (size > voxels_min)
    rank = np.cumsum(keep) - keep
    kept = np.where(keep[root], rank[root], -1)
    pv = np.asarray(point_voxel)
    return dict(connect_cross=cross, connect_final=L, attach=attach, candidates=candidates, eligible=eligible, out_of_range=out_of_range,
                root=root, size=size[root], kept=kept, point_labels=np.where(pv >= 0, kept[np.maximum(pv, 0)], -1),
                counts=dict(clusters=int(is_root.sum()), kept=int(keep.sum()), isolated=len(candidates), reattached=int((attach >= 0).sum())))


def ties(eligible, target):
    """Of one candidate: how many eligible entries carry the bit-equal maximal weight, and whether `target` is the last of them in scan order."""
    w = np.array([e[2] for e in eligible], dtype=np.float32)
    top = np.flatnonzero(w.view(np.uint32) == w.max().view(np.uint32))
    return top.size, eligible[top[-1]][1] == target
