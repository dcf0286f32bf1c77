"""The numpy restatement of absorbing small parts (tests/label_absorb_ref.py) on synthetic lattices where the answer is known by hand:
4-neighbour rows, four points per node; and the rule's invariants on random labellings of random sparse graphs."""
import numpy as np

from label_absorb_ref import absorb

PER = 4   # points per node


def _lattice(w, h):
    """offsets, idx of a w x h lattice (node = y * w + x; each row holds the node itself and its 4-neighbours), and the used flags"""
    offsets, idx = [0], []
    for y in range(h):
        for x in range(w):
            idx.append(y * w + x)
            for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                if 0 <= x + dx < w and 0 <= y + dy < h:
                    idx.append((y + dy) * w + x + dx)
            offsets.append(len(idx))
    return np.array(offsets, np.int64), np.array(idx, np.int32), np.ones(w * h, bool)


def _run(node_labels, w, h, **kw):
    off, idx, used = _lattice(w, h)
    node_labels = np.asarray(node_labels, np.int32).reshape(-1)
    labels = np.repeat(node_labels, PER)
    node = np.repeat(np.arange(w * h), PER)
    before = labels.copy()
    out = absorb(labels, node, off, idx, used, int(node_labels.max()) + 1, **kw)
    assert (labels == before).all()   # the input is unchanged
    assert (out["labels"].reshape(-1, PER) == out["labels"].reshape(-1, PER)[:, :1]).all()
    return out, out["labels"][::PER].tolist()


def test_island():
    lab = np.zeros((6, 6), np.int32)   # [y, x]
    lab[:, 3:] = 1
    clean = lab.copy()
    lab[2, 1] = 1                      # node (2, 1): row 2, column 1, inside the half of label 0
    out, got = _run(lab, 6, 6, min_points=0, island_points=10)
    assert got == clean.reshape(-1).tolist()
    assert (out["rounds"], out["parts_absorbed"], out["points_relabelled"]) == (1, 1, 4)
    assert (out["candidates_left"], out["points_dropped"], out["n_parts"]) == (0, 0, 2)
    # the comparison is strict
    out, got = _run(lab, 6, 6, min_points=0, island_points=4)
    assert got == lab.reshape(-1).tolist() and out["rounds"] == 0 and out["candidates_left"] == 0 and out["n_parts"] == 3
    out, got = _run(lab, 6, 6, min_points=0, island_points=5)
    assert got == clean.reshape(-1).tolist() and out["rounds"] == 1


def test_chain():
    lab = [0] * 10 + [1, 2]
    out, got = _run(lab, 12, 1, min_points=8)
    assert got == [0] * 12
    assert (out["rounds"], out["parts_absorbed"], out["points_relabelled"], out["n_parts"]) == (2, 2, 8, 1)
    out, got = _run(lab, 12, 1, min_points=8, max_rounds=1)
    assert got == [0] * 11 + [2]
    assert (out["rounds"], out["candidates_left"], out["candidate_points_left"], out["points_dropped"]) == (1, 1, 4, 0)
    out, got = _run(lab, 12, 1, min_points=8, max_rounds=1, drop=True)
    assert got == [0] * 11 + [-1] and (out["rounds"], out["points_dropped"]) == (1, 4)
    out, got = _run(lab, 12, 1, min_points=8, max_rounds=0, drop=True)
    assert got == [0] * 10 + [-1, -1] and (out["rounds"], out["points_dropped"], out["candidates_left"]) == (0, 8, 2)


def test_tie():
    # contacts and points equal: the lower part id
    out, got = _run([0, 0, 0, 1, 2, 2, 2], 7, 1, min_points=8)
    assert got == [0, 0, 0, 0, 2, 2, 2] and out["rounds"] == 1
    # contacts equal: the bigger part
    out, got = _run([0, 0, 1, 2, 2, 2, 2], 7, 1, min_points=8)
    assert got == [0, 0, 2, 2, 2, 2, 2] and out["rounds"] == 1


def test_shared_node_only():
    off, idx, used = np.array([0, 1], np.int64), np.array([0], np.int32), np.ones(1, bool)
    trace = []
    out = absorb(np.array([0, 0, 0, 1], np.int32), np.zeros(4, np.int64), off, idx, used, 2, min_points=2, trace=trace)
    assert out["labels"].tolist() == [0, 0, 0, 0]
    assert (out["rounds"], out["parts_absorbed"], out["points_relabelled"], out["n_parts"]) == (1, 1, 1, 1)
    assert trace[0][3].tolist() == [0, 1]   # one record: the shared node, no contact


def test_nothing_stable():
    lab = [0, 1, 2, 0, 1, 2, 0]
    out, got = _run(lab, 7, 1, min_points=8)
    assert got == lab
    assert (out["rounds"], out["candidates_left"], out["candidate_points_left"], out["points_dropped"]) == (0, 7, 28, 0)
    out, got = _run(lab, 7, 1, min_points=8, drop=True)
    assert got == [-1] * 7 and out["points_dropped"] == 28 and out["rounds"] == 0


def test_demoted_non_largest_part():
    out, got = _run([0, 0, 0, 1, 0, 0, 2], 7, 1, min_points=0, island_points=100)
    assert got == [0, 0, 0, 1, 1, 1, 2]
    assert (out["rounds"], out["parts_absorbed"], out["points_relabelled"]) == (1, 1, 8)


def test_invariants_on_random_labellings():
    rng = np.random.default_rng(11)
    for trial in range(200):
        n_nodes = int(rng.integers(1, 14))
        rows = [rng.integers(0, n_nodes, size=int(rng.integers(0, 3))).tolist() for _ in range(n_nodes)]
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        idx = np.array([w for r in rows for w in r], np.int32)
        used = np.ones(n_nodes, bool)
        n = int(rng.integers(0, 40))
        K = int(rng.integers(1, 4))
        labels = rng.integers(-1, K, size=n).astype(np.int32)
        node = rng.integers(-1, n_nodes, size=n)
        before = labels.copy()
        kw = dict(min_points=int(rng.integers(0, 6)), island_points=int(rng.integers(0, 8)))
        # default parameters: the identity
        same = absorb(labels, node, off, idx, used, K)
        assert (same["labels"] == labels).all() and same["rounds"] == 0 and same["candidates_left"] == 0
        # C strictly falls per applied round
        trace = []
        out = absorb(labels, node, off, idx, used, K, max_rounds=64, trace=trace, **kw)
        Cs = [t[0]["n_parts"] for t in trace]
        assert len(Cs) == out["rounds"] + 1 and all(a > b for a, b in zip(Cs, Cs[1:]))
        # ended before the cap without drop: no remaining candidate has a stable neighbour
        assert (trace[-1][2] < 0).all()
        # with drop the output has no candidate when evaluated again
        dropped = absorb(labels, node, off, idx, used, K, max_rounds=int(rng.integers(0, 3)), drop=True, **kw)
        again = absorb(dropped["labels"], node, off, idx, used, K, max_rounds=0, **kw)
        assert again["candidates_left"] == 0
        # points outside the pass keep their label
        outside = (labels >= 0) & (node < 0)
        assert (dropped["labels"][outside] == labels[outside]).all() and dropped["n_skipped"] == int(outside.sum())
        assert (labels == before).all()
