"""Plain numpy restatement of absorbing the stranded and the small parts of a per-point labelling (include/vgs.h,
vgs_absorb_point_label_parts), the reference of tests/test_gpu_label_absorb.py.

Built only from label_components_ref.label_components and label_graph_ref.label_graph (weight=None) plus a plain loop; no engine, no
shared code.  Inputs as theirs: the labels, the node of every point, the rows of every node as CSR, the used flags, K."""
import numpy as np

from label_components_ref import label_components
from label_graph_ref import label_graph

COUNTS = ("rounds", "parts_absorbed", "points_relabelled", "candidates_left", "candidate_points_left", "points_dropped", "n_parts",
          "n_skipped")


def evaluate(labels, node, off, idx, used, K, min_points, island_points):
    """one EVALUATION: the parts, the candidate flags, the target of every part (-1: none) and the number of (candidate, stable
    neighbour) records of every part"""
    cmp = label_components(labels, node, off, idx, K)
    C = cmp["n_parts"]
    g = label_graph(cmp["part_of_point"], node, off, idx, used, C, weight=None)
    pts, plab = cmp["part_points"], cmp["part_label"]
    thr = np.full(C, max(min_points, island_points), np.int64)
    for p in range(C):
        if cmp["label_largest"][plab[p]] == p:
            thr[p] = min_points
    cand = pts < thr
    best = [None] * C
    n_rec = np.zeros(C, np.int64)
    for e in range(g["n_edges"]):
        a, b = (int(x) for x in g["seg_ab"][e])
        assert plab[a] != plab[b]   # parts of one label are never adjacent
        score = int(g["n_shared"][e]) + int(g["n_pairs"][e])
        for p, q in ((a, b), (b, a)):
            if cand[p] and not cand[q]:
                n_rec[p] += 1
                t = (score, int(pts[q]), -q)
                if best[p] is None or t > best[p]:
                    best[p] = t
    target = np.array([-1 if t is None else -t[2] for t in best], np.int64).reshape(C)
    return cmp, cand, target, n_rec


def absorb(labels, node, off, idx, used, K, min_points=0, island_points=0, max_rounds=8, drop=False, trace=None):
    """the dict of Engine.absorb_label_parts: labels (int32) and the eight counts by name.  trace: a list that receives (cmp, cand,
    target, n_rec) of every evaluation"""
    lab = np.array(labels, dtype=np.int32).reshape(-1)
    rounds = absorbed = moved = 0
    r = 0
    while True:
        cmp, cand, target, n_rec = evaluate(lab, node, off, idx, used, K, min_points, island_points)
        if trace is not None:
            trace.append((cmp, cand, target, n_rec))
        P = cmp["part_of_point"]
        if r == max_rounds or not (target >= 0).any():
            break
        has = P >= 0
        t = np.full(lab.shape[0], -1, np.int64)
        t[has] = target[P[has]]
        go = t >= 0
        lab = lab.copy()
        lab[go] = cmp["part_label"][t[go]]
        rounds += 1
        absorbed += int((target >= 0).sum())
        moved += int(go.sum())
        r += 1
    dropped = 0
    if drop:
        gone = np.zeros(lab.shape[0], bool)
        gone[P >= 0] = cand[P[P >= 0]]
        lab = lab.copy()
        lab[gone] = -1
        dropped = int(gone.sum())
    out = {"labels": lab, "rounds": rounds, "parts_absorbed": absorbed, "points_relabelled": moved, "candidates_left": int(cand.sum()),
           "candidate_points_left": int(cmp["part_points"][cand].sum()), "points_dropped": dropped, "n_parts": int(cmp["n_parts"]),
           "n_skipped": int(cmp["n_skipped"])}
    return out


def diff(got, ref):
    """the names in which two results differ ([] = none): the label array byte for byte, the counts as integers"""
    g, r = np.asarray(got["labels"]), np.asarray(ref["labels"])
    bad = [] if (g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()) else ["labels"]
    return bad + [k for k in COUNTS if int(got[k]) != int(ref[k])]
