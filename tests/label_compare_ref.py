"""Numpy restatement of the label comparison (include/vgs.h: vgs_compare_labels, vgs_get_label_comparison): the sparse contingency table
between point labels and a reference labelling, the reference table, the segment table and the summary, straight from the definitions.
Everything is an integer or one fp64 division of two integers, so the engine's tables must equal these bit for bit.
compare_brute() says the same with plain loops over points and dictionaries (small clouds only); scores_formulas() writes the scores of
api.comparison_scores out independently."""
import math

import numpy as np

FIELDS = (("cell_seg", np.int32), ("cell_ref", np.int32), ("cell_n", np.int64),
          ("ref_id", np.int32), ("ref_points", np.int64), ("ref_dropped", np.int64), ("ref_best_seg", np.int32), ("ref_best_n", np.int64),
          ("ref_best_iou", np.float64),
          ("seg_annotated", np.int64), ("seg_refs", np.int32), ("seg_best_ref", np.int32), ("seg_best_n", np.int64), ("seg_best_iou", np.float64),
          ("summary", np.int64))


def _pairs(a):
    a = np.asarray(a, dtype=np.int64)
    return a * (a - 1) // 2


def compare_labels(labels, ref, K):
    """The dict of Engine.compare_labels for point labels `labels` (-1 .. K-1) and reference ids `ref` (negative: not annotated)."""
    L = np.asarray(labels).astype(np.int64)
    g = np.asarray(ref).astype(np.int64)
    assert L.shape == g.shape and L.ndim == 1
    ann = g >= 0
    L, g = L[ann], g[ann]
    key, cell_n = np.unique((L + 1) * (1 << 31) + g, return_counts=True)   # ascending (L, g), the -1 row first
    cell_seg, cell_ref = key // (1 << 31) - 1, key % (1 << 31)
    cell_n = cell_n.astype(np.int64)
    kept = cell_seg >= 0
    # segment table
    seg_annotated = np.zeros(K, np.int64)
    np.add.at(seg_annotated, cell_seg[kept], cell_n[kept])
    seg_refs = np.bincount(cell_seg[kept], minlength=K).astype(np.int64)[:K] if K else np.zeros(0, np.int64)
    seg_best_ref, seg_best_n = np.full(K, -1, np.int64), np.zeros(K, np.int64)
    for i in np.flatnonzero(kept):   # ascending id inside a row: a strictly larger count only
        k = cell_seg[i]
        if cell_n[i] > seg_best_n[k]:
            seg_best_n[k], seg_best_ref[k] = cell_n[i], cell_ref[i]
    # reference table
    ref_id = np.unique(cell_ref)
    G = ref_id.size
    row = np.searchsorted(ref_id, cell_ref)
    ref_points, ref_dropped = np.zeros(G, np.int64), np.zeros(G, np.int64)
    np.add.at(ref_points, row, cell_n)
    np.add.at(ref_dropped, row[~kept], cell_n[~kept])
    ref_best_seg, ref_best_n = np.full(G, -1, np.int64), np.zeros(G, np.int64)
    for i in np.flatnonzero(kept):   # the cells come in ascending label: a strictly larger count only
        r = row[i]
        if cell_n[i] > ref_best_n[r]:
            ref_best_n[r], ref_best_seg[r] = cell_n[i], cell_seg[i]
    ref_best_iou = np.zeros(G, np.float64)
    h = ref_best_seg >= 0
    ref_best_iou[h] = ref_best_n[h].astype(np.float64) / (seg_annotated[ref_best_seg[h]] + ref_points[h] - ref_best_n[h]).astype(np.float64)
    seg_best_iou = np.zeros(K, np.float64)
    h = seg_best_ref >= 0
    rp = ref_points[np.searchsorted(ref_id, seg_best_ref[h])]
    seg_best_iou[h] = seg_best_n[h].astype(np.float64) / (seg_annotated[h] + rp - seg_best_n[h]).astype(np.float64)
    dropped = int(cell_n[~kept].sum())
    summary = np.array([L.size, int((~ann).sum()), dropped, G, key.size, int((seg_annotated > 0).sum()), int(seg_best_n.sum()),
                        int(ref_best_n.sum()), int(_pairs(cell_n).sum()), int(_pairs(seg_annotated).sum()) + int(_pairs(dropped)),
                        int(_pairs(ref_points).sum()), 0], np.int64)
    out = dict(cell_seg=cell_seg, cell_ref=cell_ref, cell_n=cell_n, ref_id=ref_id, ref_points=ref_points, ref_dropped=ref_dropped,
               ref_best_seg=ref_best_seg, ref_best_n=ref_best_n, ref_best_iou=ref_best_iou, seg_annotated=seg_annotated, seg_refs=seg_refs,
               seg_best_ref=seg_best_ref, seg_best_n=seg_best_n, seg_best_iou=seg_best_iou, summary=summary)
    return {name: np.asarray(out[name]).astype(dt) for name, dt in FIELDS}


def compare_brute(labels, ref, K):
    """The same tables by loops over the points and over all (segment, id) pairs: nothing sorted, nothing shared with compare_labels."""
    labels, ref = [int(v) for v in labels], [int(v) for v in ref]
    n_ann = sum(1 for r in ref if r >= 0)
    cells = {}
    for L, r in zip(labels, ref):
        if r >= 0:
            cells[(L, r)] = cells.get((L, r), 0) + 1
    order = sorted(cells)
    ids = sorted({r for r in ref if r >= 0})
    ref_points = [sum(1 for r in ref if r == i) for i in ids]
    ref_dropped = [sum(1 for L, r in zip(labels, ref) if r == i and L < 0) for i in ids]
    seg_annotated = [sum(1 for L, r in zip(labels, ref) if L == k and r >= 0) for k in range(K)]
    seg_refs = [len({r for L, r in zip(labels, ref) if L == k and r >= 0}) for k in range(K)]
    seg_best_ref, seg_best_n, seg_best_iou = [], [], []
    for k in range(K):
        best, arg = 0, -1
        for i in ids:
            c = cells.get((k, i), 0)
            if c > best:
                best, arg = c, i
        seg_best_ref.append(arg)
        seg_best_n.append(best)
        seg_best_iou.append(best / (seg_annotated[k] + ref_points[ids.index(arg)] - best) if arg >= 0 else 0.0)
    ref_best_seg, ref_best_n, ref_best_iou = [], [], []
    for j, i in enumerate(ids):
        best, arg = 0, -1
        for k in range(K):
            c = cells.get((k, i), 0)
            if c > best:
                best, arg = c, k
        ref_best_seg.append(arg)
        ref_best_n.append(best)
        ref_best_iou.append(best / (seg_annotated[arg] + ref_points[j] - best) if arg >= 0 else 0.0)
    dropped = sum(1 for L, r in zip(labels, ref) if L < 0 and r >= 0)
    c2 = lambda a: a * (a - 1) // 2   # noqa: E731
    summary = [n_ann, len(ref) - n_ann, dropped, len(ids), len(order), sum(1 for a in seg_annotated if a > 0), sum(seg_best_n), sum(ref_best_n),
               sum(c2(v) for v in cells.values()), sum(c2(a) for a in seg_annotated) + c2(dropped), sum(c2(p) for p in ref_points), 0]
    out = dict(cell_seg=[k for k, _ in order], cell_ref=[r for _, r in order], cell_n=[cells[o] for o in order], ref_id=ids,
               ref_points=ref_points, ref_dropped=ref_dropped, ref_best_seg=ref_best_seg, ref_best_n=ref_best_n, ref_best_iou=ref_best_iou,
               seg_annotated=seg_annotated, seg_refs=seg_refs, seg_best_ref=seg_best_ref, seg_best_n=seg_best_n, seg_best_iou=seg_best_iou,
               summary=summary)
    return {name: np.asarray(out[name], dtype=dt).reshape(-1) for name, dt in FIELDS}


def same(a, b):
    """every array of two comparison dicts equal, dtype and bytes"""
    return all(a[n].dtype == b[n].dtype == dt and a[n].shape == b[n].shape and a[n].tobytes() == b[n].tobytes() for n, dt in FIELDS)


def diff(a, b):
    """the names of the arrays that differ (for assertion messages)"""
    return [n for n, dt in FIELDS if not (a[n].dtype == b[n].dtype == dt and a[n].shape == b[n].shape and a[n].tobytes() == b[n].tobytes())]


def scores_formulas(cmp, tau):
    """The scores of api.comparison_scores written out from the issue's formulas in exact rational arithmetic where that is possible"""
    from fractions import Fraction
    s = [int(v) for v in cmp["summary"]]
    nan = float("nan")
    matched = sum(1 for v in cmp["seg_best_iou"] if v > tau)
    P = Fraction(matched, s[5]) if s[5] else None
    R = Fraction(matched, s[3]) if s[3] else None
    f1 = nan if P is None or R is None or P + R == 0 else float(2 * P * R / (P + R))
    n = s[0]
    T = n * (n - 1) // 2
    if T == 0:
        ari = nan
    else:
        e = Fraction(s[9] * s[10], T)
        den = Fraction(s[9] + s[10], 2) - e
        ari = float((s[8] - e) / den) if den != 0 else nan
    return {"matched": matched, "precision": nan if P is None else float(P), "recall": nan if R is None else float(R), "f1": f1,
            "purity": s[6] / (s[0] - s[2]) if s[0] - s[2] else nan, "completeness": s[7] / s[0] if s[0] else nan, "ari": ari}


def close(a, b, rel=1e-12):
    return (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= rel * max(abs(a), abs(b))
