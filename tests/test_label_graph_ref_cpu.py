"""tests/label_graph_ref.py, the numpy restatement of vgs_point_label_graph's definition, against a double loop over vertex pairs on seeded
random graphs with several labels per node, asymmetric rows and unused nodes; and against helpers.graph_truth where every node carries one
label.  No GPU."""
import numpy as np
import pytest

import helpers
import label_graph_ref as R


def _random_graph(seed, V=70, K=12, symmetric=False):
    rng = np.random.default_rng(seed)
    adj = rng.random((V, V)) < 0.08
    np.fill_diagonal(adj, False)
    if symmetric:
        adj = adj | adj.T
    rows = [[v] + np.nonzero(adj[v])[0].tolist() for v in range(V)]   # a row starts with its own node, as the stored rows do
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int32)
    used = rng.random(V) < 0.8
    w = rng.random((V, V)).astype(np.float32)
    w[rng.random((V, V)) < 0.1] = np.nan
    return rng, adj, off, idx, used, w


def _loop(labels, pv, adj, used, K, w):
    """the definition, one vertex pair at a time"""
    verts = sorted({(int(l), int(v)) for l, v in zip(labels, pv) if l >= 0 and v >= 0})
    edges = {}

    def edge(a, b):
        return edges.setdefault((a, b), dict(n_shared=0, n_pairs=0, n_finite=0, va=set(), vb=set(), ws=[]))

    for i, (a, v) in enumerate(verts):
        for b, x in verts[i + 1:]:
            if a == b:
                continue   # (a < b from here on: the vertices are sorted by label first)
            if v == x:
                edge(a, b)["n_shared"] += 1
            elif adj[v, x] or adj[x, v]:
                e = edge(a, b)
                e["n_pairs"] += 1
                e["va"].add(v)
                e["vb"].add(x)
                if used[v] and used[x]:
                    ww = w[min(v, x), max(v, x)]
                    if not np.isnan(ww):
                        e["n_finite"] += 1
                        e["ws"].append(ww)
    keys = sorted(edges)
    E = len(keys)
    return dict(seg_ab=np.array(keys, np.int32).reshape(E, 2), n_shared=np.array([edges[k]["n_shared"] for k in keys], np.int64),
                n_pairs=np.array([edges[k]["n_pairs"] for k in keys], np.int64), n_finite=np.array([edges[k]["n_finite"] for k in keys], np.int64),
                nodes_ab=np.array([[len(edges[k]["va"]), len(edges[k]["vb"])] for k in keys], np.int32).reshape(E, 2),
                w_sum=np.array([np.sum(np.array(edges[k]["ws"], np.float64)) for k in keys], np.float64),
                w_min=np.array([min(edges[k]["ws"]) if edges[k]["ws"] else np.nan for k in keys], np.float32),
                w_max=np.array([max(edges[k]["ws"]) if edges[k]["ws"] else np.nan for k in keys], np.float32),
                n_edges=E, n_skipped=int(((labels >= 0) & (pv < 0)).sum()))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_restatement_against_a_double_loop(seed):
    V, K = 70, 12
    rng, adj, off, idx, used, w = _random_graph(seed, V, K)
    per = rng.integers(1, 5, size=V)   # 1 to 4 labels per node (fewer where two draws coincide)
    pv = np.repeat(np.arange(V), per * 2)
    labels = rng.integers(0, K, size=pv.shape[0])
    labels[rng.random(pv.shape[0]) < 0.1] = -1
    pv = np.concatenate([pv, [-1, -1, -1]])   # points without a node: one unlabelled, two labelled
    labels = np.concatenate([labels, [-1, 3, 5]])
    ref = _loop(labels, pv, adj, used, K, w)
    got = R.label_graph(labels, pv, off, idx, used, K, lambda a, b: w[a, b])
    assert R.diff(got, ref) == [], R.diff(got, ref)
    assert got["n_skipped"] == 2 and got["n_edges"] > 10 and (got["n_shared"] > 0).any() and (got["n_finite"] < got["n_pairs"]).any()
    counts = R.label_graph(labels, pv, off, idx, used, K)   # without weights: the integer fields alone
    assert "w_sum" not in counts and R.diff(counts, {k: ref[k] for k in ("seg_ab", "n_shared", "n_pairs", "nodes_ab")}) == []


@pytest.mark.parametrize("seed", [5, 6])
def test_one_label_per_node_equals_graph_truth(seed):
    V, K = 70, 12
    rng, adj, off, idx, used, w = _random_graph(seed, V, K, symmetric=True)   # graph_truth asks for symmetric rows
    node_label = rng.integers(0, K, size=V)
    eff = np.where(used, node_label, -1)   # unused nodes unlabelled
    pv = np.repeat(np.arange(V), 3)
    labels = eff[pv]
    truth = helpers.graph_truth(eff, off, idx, K, lambda a, b: w[a, b])
    got = R.label_graph(labels, pv, off, idx, used, K, lambda a, b: w[a, b])
    assert got["n_edges"] == truth["seg_ab"].shape[0] > 5 and (got["n_shared"] == 0).all()
    assert R.diff(got, {k: truth[k] for k in ("seg_ab", "n_pairs", "n_finite", "nodes_ab", "w_sum", "w_min", "w_max")}) == []


def test_degenerate_inputs():
    off, idx, used = np.zeros(4, np.int64), np.zeros(0, np.int32), np.ones(3, bool)
    for labels, K in ((np.array([-1, -1]), 0), (np.array([0, 0]), 1), (np.array([-1, -1]), 5)):
        got = R.label_graph(labels, np.array([0, 1]), off, idx, used, K, lambda a, b: np.zeros(a.shape[0], np.float32))
        assert got["n_edges"] == 0 and all(np.asarray(got[k]).shape[0] == 0 for k in R.FIELDS)
