"""The element order of the reference's connect lists, restated in plain numpy and Python (no engine, no oracle): what
csrc/cutorder.hip recomputes on the device and vgs_get_lists_ordered(..., VGS_ORDER_REFERENCE, ...) returns.

cut_order scans EVERY pair of the row, as cutGraphSegmentation does; the kernels replay the scan inside the connect set S0 only, and
that shortcut is part of what the comparison tests.  tests/test_cut_order_ref_cpu.py pins cut_order to the oracle's lean cut."""
import numpy as np


def cut_order(W, cut):
    """The vertex list of the segment that holds vertex 0, in merge-history order, as row positions.

    W: the n x n float32 matrix of one node (Engine.local_weights; row and column 0 are the node itself).  Edges are the pairs a < b with
    a non-NaN W[a, b], scanned by (w descending, a ascending, b ascending).  Every vertex starts as its own segment with the threshold
    1 - cut / 1; an edge merges the segments A (of a) and B (of b) only if w > thr[A] and w > thr[B]; the survivor is A if
    thr[A] >= thr[B], else B; it gets the absorbed segment's vertices appended and the threshold w - cut / size.  All in float32."""
    W = np.asarray(W, dtype=np.float32)
    n = W.shape[0]
    assert W.shape == (n, n) and n >= 1
    a, b = np.triu_indices(n, 1)             # row-major over a < b
    w = W[a, b]
    ok = ~np.isnan(w)
    a, b, w = a[ok], b[ok], w[ok]
    order = np.lexsort((b, a, -w))           # last key first: w descending, then a, then b
    a, b, w = a[order], b[order], w[order]
    one, c = np.float32(1), np.float32(cut)
    seg = list(range(n))
    members = [[v] for v in range(n)]
    thr = [float(one - c / one)] * n         # float32 values held as Python floats: comparisons are exact
    for wi, ai, bi in zip(w.tolist(), a.tolist(), b.tolist()):
        A, B = seg[ai], seg[bi]
        if A == B:
            continue
        if not (wi > thr[A] and wi > thr[B]):
            continue
        keep, gone = (A, B) if thr[A] >= thr[B] else (B, A)
        for v in members[gone]:
            seg[v] = keep
        members[keep] += members[gone]
        members[gone] = []
        thr[keep] = float(np.float32(wi) - c / np.float32(len(members[keep])))
    return list(members[seg[0]])


def cross_order(cut_list_u, u, cut_sets):
    """crossValidation: the entries v of u's list with u in v's own list (cut_sets[v]: any container), in list order."""
    return [int(v) for v in cut_list_u if u in cut_sets[int(v)]]


def final_order(cross_lists, attach):
    """closestCheck's appends: for i ascending with a target t = attach[i] >= 0, L[i] += [t] and L[t] += [i]."""
    L = [list(l) for l in cross_lists]
    for i, t in enumerate(attach):
        t = int(t)
        if t >= 0:
            L[i].append(t)
            L[t].append(i)
    return L
