"""The numpy restatement of the connected parts of a point labelling (tests/label_components_ref.py) against
scipy.sparse.csgraph.connected_components on hand-made graphs, and the numbering rule on each: parts in ascending (label, smallest node
id of the part), so that the parts of a label are a contiguous range."""
import numpy as np
from scipy import sparse
from scipy.sparse import csgraph

from label_components_ref import label_components


def _rows(n_nodes, rows):
    """offsets, idx of Engine.lists(0) from {node: [neighbours]}"""
    offsets, idx = [0], []
    for v in range(n_nodes):
        idx += list(rows.get(v, []))
        offsets.append(len(idx))
    return np.array(offsets, np.int64), np.array(idx, np.int32)


def _by_scipy(labels, node, offsets, idx, K):
    """(sorted list of frozensets of point indices, one per part; their labels) from scipy over the (label, node) vertices"""
    labels, node = np.asarray(labels), np.asarray(node)
    n_nodes = offsets.size - 1
    live = np.flatnonzero((labels >= 0) & (node >= 0))
    verts = sorted({(int(labels[i]), int(node[i])) for i in live})
    at = {lv: k for k, lv in enumerate(verts)}
    r, c = [], []
    for (l, v), k in at.items():
        for w in idx[offsets[v]:offsets[v + 1]]:
            if (l, int(w)) in at:
                r.append(k), c.append(at[(l, int(w))])
    g = sparse.coo_matrix((np.ones(len(r)), (r, c)), shape=(len(verts), len(verts)))
    n, comp = csgraph.connected_components(g, directed=True, connection="weak") if verts else (0, np.zeros(0, int))
    parts = {}
    for i in live:
        parts.setdefault(int(comp[at[(int(labels[i]), int(node[i]))]]), set()).add(int(i))
    assert len(parts) == n
    return list(parts.values()), n


def _check(labels, node, offsets, idx, K):
    labels, node = np.asarray(labels, np.int32), np.asarray(node, np.int32)
    got = label_components(labels, node, offsets, idx, K)
    want, n = _by_scipy(labels, node, offsets, idx, K)
    C = got["n_parts"]
    assert C == n == got["part_label"].size
    pop = got["part_of_point"]
    assert sorted(np.flatnonzero(pop == p).tolist() for p in range(C)) == sorted(map(sorted, want))
    live = (labels >= 0) & (node >= 0)
    assert (pop[~live] == -1).all() and (pop[live] >= 0).all()
    assert got["n_skipped"] == int(((labels >= 0) & (node < 0)).sum())
    # the tables against the point ids
    for p in range(C):
        m = pop == p
        assert set(labels[m]) == {got["part_label"][p]}
        assert got["part_points"][p] == m.sum()
        assert got["part_nodes"][p] == np.unique(node[m]).size
        assert got["part_first_node"][p] == node[m].min()
    # the numbering rule: ascending (label, smallest node), strictly
    order = list(zip(got["part_label"].tolist(), got["part_first_node"].tolist()))
    assert order == sorted(order) and len(set(order)) == C
    lf = got["label_first"]
    assert lf.shape == (K + 1,) and lf[0] == 0 and lf[K] == C and (np.diff(lf) >= 0).all()
    for k in range(K):
        assert (got["part_label"][lf[k]:lf[k + 1]] == k).all()
        rng = np.arange(lf[k], lf[k + 1])
        if rng.size == 0:
            assert got["label_largest"][k] == -1
        else:
            pts = got["part_points"][rng]
            assert got["label_largest"][k] == rng[np.flatnonzero(pts == pts.max())[0]]
    return got


def test_a_path_is_one_part():
    offsets, idx = _rows(5, {v: [w for w in (v - 1, v, v + 1) if 0 <= w < 5] for v in range(5)})
    node = np.repeat(np.arange(5), 3)
    got = _check(np.zeros(15, np.int32), node, offsets, idx, 1)
    assert got["n_parts"] == 1 and got["part_nodes"].tolist() == [5] and got["part_points"].tolist() == [15]
    assert got["label_first"].tolist() == [0, 1] and got["label_largest"].tolist() == [0]


def test_two_islands_of_one_label():
    offsets, idx = _rows(6, {0: [1], 1: [0], 2: [], 3: [], 4: [5], 5: [4]})
    node = np.array([0, 1, 1, 4, 5, 5, 5, 2, 3])
    labels = np.array([0, 0, 0, 0, 0, 0, 0, -1, 1], np.int32)
    got = _check(labels, node, offsets, idx, 2)
    assert got["n_parts"] == 3 and got["part_label"].tolist() == [0, 0, 1] and got["part_first_node"].tolist() == [0, 4, 3]
    assert got["part_points"].tolist() == [3, 4, 1] and got["label_largest"].tolist() == [1, 2]
    assert got["part_of_point"].tolist() == [0, 0, 0, 1, 1, 1, 1, -1, 2]


def test_two_labels_alternating_inside_every_node():
    offsets, idx = _rows(4, {0: [1], 1: [0, 2], 2: [1], 3: []})
    node = np.repeat(np.arange(4), 4)
    labels = (np.arange(16) % 2).astype(np.int32)
    got = _check(labels, node, offsets, idx, 2)
    # per label: nodes 0-1-2 one part, node 3 another; label 0's parts come first
    assert got["part_label"].tolist() == [0, 0, 1, 1] and got["part_first_node"].tolist() == [0, 3, 0, 3]
    assert got["part_nodes"].tolist() == [3, 1, 3, 1] and got["label_first"].tolist() == [0, 2, 4]


def test_a_one_directional_row_entry_still_joins():
    offsets, idx = _rows(3, {0: [], 1: [0], 2: []})   # only node 1's row names node 0
    got = _check(np.zeros(3, np.int32), np.arange(3), offsets, idx, 1)
    assert got["n_parts"] == 2 and got["part_nodes"].tolist() == [2, 1] and got["part_of_point"].tolist() == [0, 0, 1]
    # and from the other side alone
    offsets, idx = _rows(3, {0: [1], 1: [], 2: []})
    assert _check(np.zeros(3, np.int32), np.arange(3), offsets, idx, 1)["part_of_point"].tolist() == [0, 0, 1]


def test_an_empty_label_between_two_used_ones_and_a_tie():
    offsets, idx = _rows(4, {0: [1], 1: [0], 2: [], 3: []})
    node = np.array([0, 1, 2, 3, -1])
    labels = np.array([2, 2, 0, 0, 2], np.int32)   # label 0: two parts of one point (a tie), label 1: none, label 2: one part; one skipped point
    got = _check(labels, node, offsets, idx, 4)
    assert got["part_label"].tolist() == [0, 0, 2] and got["label_first"].tolist() == [0, 2, 2, 3, 3]
    assert got["label_largest"].tolist() == [0, -1, 2, -1] and got["n_skipped"] == 1 and got["part_of_point"][4] == -1


def test_k_zero_and_no_points():
    offsets, idx = _rows(2, {0: [1], 1: [0]})
    got = _check(np.array([-1, -5], np.int32), np.array([0, 1]), offsets, idx, 0)
    assert got["n_parts"] == 0 and got["label_first"].tolist() == [0] and got["label_largest"].size == 0
    assert got["part_of_point"].tolist() == [-1, -1]
    got = _check(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), 3)
    assert got["n_parts"] == 0 and got["label_first"].tolist() == [0, 0, 0, 0] and got["label_largest"].tolist() == [-1, -1, -1]


def test_random_graphs_agree_with_scipy():
    rng = np.random.default_rng(5)
    for trial in range(20):
        n_nodes = int(rng.integers(1, 40))
        rows = {v: rng.integers(0, n_nodes, size=int(rng.integers(0, 4))).tolist() for v in range(n_nodes)}
        offsets, idx = _rows(n_nodes, rows)
        n = int(rng.integers(0, 200))
        K = int(rng.integers(1, 5))
        _check(rng.integers(-1, K, size=n).astype(np.int32), rng.integers(-1, n_nodes, size=n), offsets, idx, K)
