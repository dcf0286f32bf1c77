"""CPU tests of the edge fold of the tiled driver (vgs_tiles_fold_edges, csrc/tiles.cpp): random per-rank partial edge tables as
vgs_get_own_segment_graph gives them -- edges on one, several or all ranks, ranks without a finite weight (NaN min and max), an empty
rank, more than 65 536 labels -- against a restatement of the rules of include/vgs_tiles.h in plain Python: counts, min and max exact,
w_sum bit-identical (the same order of the same fp64 additions)."""
import numpy as np
import pytest

FIELDS = ("seg_ab", "n_pairs", "n_finite", "nodes_ab", "w_sum", "w_min", "w_max")


@pytest.fixture(scope="module")
def tn(vgs):
    from vgs_svgs_segmentation_amd import tiles_native
    tiles_native.lib()
    return tiles_native


def _table(rows):
    """rows: (a, b, n_pairs, n_finite, nodes_a, nodes_b, w_sum, w_min, w_max), any order -> one rank's table, ascending (a, b)"""
    rows = sorted(rows, key=lambda r: (r[0], r[1]))
    n = len(rows)
    return {"seg_ab": np.array([r[0:2] for r in rows], dtype=np.int32).reshape(n, 2), "n_pairs": np.array([r[2] for r in rows], dtype=np.int64),
            "n_finite": np.array([r[3] for r in rows], dtype=np.int64), "nodes_ab": np.array([r[4:6] for r in rows], dtype=np.int32).reshape(n, 2),
            "w_sum": np.array([r[6] for r in rows], dtype=np.float64), "w_min": np.array([r[7] for r in rows], dtype=np.float32),
            "w_max": np.array([r[8] for r in rows], dtype=np.float32)}


def _random_tables(rng, world, K, n_edges, empty_rank=None):
    """a pool of n_edges label pairs; every rank holds a random subset of it (the first three pairs: one rank, two ranks, every rank), and
    about a third of a rank's edges have no finite weight there"""
    pool = set()
    while len(pool) < n_edges:
        a, b = sorted(int(x) for x in rng.integers(0, K, 2))
        if a != b:
            pool.add((a, b))
    pool = sorted(pool)
    holders = []
    for i, _ in enumerate(pool):
        if i == 0:
            h = [world - 1]
        elif i == 1:
            h = [0, world - 1] if world > 1 else [0]
        elif i == 2:
            h = list(range(world))
        else:
            h = [r for r in range(world) if rng.random() < 0.5] or [int(rng.integers(0, world))]
        holders.append([r for r in h if r != empty_rank] or [r for r in range(world) if r != empty_rank][:1])
    tables = []
    for r in range(world):
        rows = []
        for (a, b), h in zip(pool, holders):
            if r not in h:
                continue
            n_pairs = int(rng.integers(1, 1000))
            n_fin = 0 if rng.random() < 0.33 else int(rng.integers(1, n_pairs + 1))
            w = np.sort(rng.random(2).astype(np.float32))
            rows.append((a, b, n_pairs, n_fin, int(rng.integers(0, 50)), int(rng.integers(0, 50)), float(rng.random() * n_fin) if n_fin else 0.0,
                         w[0] if n_fin else np.nan, w[1] if n_fin else np.nan))
        tables.append(_table(rows))
    return tables


def _restate(tables, K):
    """the rules, literally: merge by (a, b); per edge, ranks ascending; counts add, w_sum adds from 0.0 in that order, min / max over the
    ranks with n_finite > 0, NaN when the total is 0"""
    edges = {}
    for r, t in enumerate(tables):
        for i in range(t["seg_ab"].shape[0]):
            edges.setdefault((int(t["seg_ab"][i, 0]), int(t["seg_ab"][i, 1])), []).append((r, i))
    rows = []
    for (a, b) in sorted(edges):
        n_pairs = n_fin = na = nb = 0
        s = np.float64(0.0)
        mn = mx = None
        for r, i in sorted(edges[(a, b)]):
            t = tables[r]
            n_pairs += int(t["n_pairs"][i]); n_fin += int(t["n_finite"][i])
            na += int(t["nodes_ab"][i, 0]); nb += int(t["nodes_ab"][i, 1])
            s = s + t["w_sum"][i]
            if t["n_finite"][i] > 0:
                mn = t["w_min"][i] if mn is None else min(mn, t["w_min"][i])
                mx = t["w_max"][i] if mx is None else max(mx, t["w_max"][i])
        rows.append((a, b, n_pairs, n_fin, na, nb, s, np.nan if mn is None else mn, np.nan if mx is None else mx))
    return _table(rows)


def _assert_same(got, ref):
    assert set(got) == set(FIELDS)
    for k in FIELDS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), k   # bit for bit, NaN included


@pytest.mark.parametrize("world,K,n_edges,empty", [(2, 40, 60, None), (4, 300, 500, 2), (8, 100_000, 2000, 5), (3, 70_000, 50, None)],
                         ids=["2", "4-empty-rank", "8-large-K", "3-large-K"])
def test_fold_equals_the_restated_rules(tn, world, K, n_edges, empty):
    rng = np.random.default_rng(100 + world)
    tables = _random_tables(rng, world, K, n_edges, empty_rank=empty)
    if empty is not None:
        assert tables[empty]["seg_ab"].shape[0] == 0
    ref = _restate(tables, K)
    got = tn.fold_edges(tables, K)
    _assert_same(got, ref)
    # the cases are there: an edge on one rank, on several, on all; a rank's NaN ignored next to a finite one; an edge with no finite weight
    per_edge = {}
    for r, t in enumerate(tables):
        for i in range(t["seg_ab"].shape[0]):
            per_edge.setdefault(tuple(t["seg_ab"][i]), []).append(int(t["n_finite"][i]))
    sizes = {len(v) for v in per_edge.values()}
    assert 1 in sizes and (world - (empty is not None)) in sizes and (world < 3 or any(1 < s < world for s in sizes))
    assert any(0 in v and max(v) > 0 for v in per_edge.values())
    assert np.isnan(got["w_min"]).any() and (np.isnan(got["w_min"]) == (got["n_finite"] == 0)).all()
    assert (np.isnan(got["w_max"]) == (got["n_finite"] == 0)).all()
    if K > 65_536:
        key = got["seg_ab"][:, 0].astype(np.int64) * K + got["seg_ab"][:, 1]
        assert key.max() >= 2 ** 32 and (np.diff(key) > 0).all()


def test_world_of_one_returns_its_input(tn):
    t = _random_tables(np.random.default_rng(7), 1, 1000, 200)
    got = tn.fold_edges(t, 1000)
    _assert_same(got, t[0])


def test_no_edges_at_all(tn):
    got = tn.fold_edges([_table([]), _table([])], 10)
    assert got["seg_ab"].shape == (0, 2) and got["w_sum"].shape == (0,)


def test_w_sum_order_is_rank_order(tn):
    """three addends whose fp64 sum depends on the order: the fold takes rank 0, then 1, then 2"""
    vals = [1.0, 1e-16, -1.0]
    tables = [_table([(0, 1, 1, 1, 1, 1, v, 0.5, 0.5)]) for v in vals]
    got = tn.fold_edges(tables, 2)
    assert got["w_sum"][0] == (np.float64(0.0) + vals[0] + vals[1]) + vals[2]
    assert got["w_sum"][0] != (np.float64(0.0) + vals[0] + vals[2]) + vals[1]


@pytest.mark.parametrize("rows,K", [([(0, 5, 1, 1, 1, 1, 0.5, 0.5, 0.5)], 5),                                        # b outside 0 .. K-1
                                    ([(-1, 2, 1, 1, 1, 1, 0.5, 0.5, 0.5)], 5),                                       # a negative
                                    ([(3, 3, 1, 1, 1, 1, 0.5, 0.5, 0.5)], 5),                                        # a == b
                                    ([(4, 2, 1, 1, 1, 1, 0.5, 0.5, 0.5)], 5)],                                       # a > b
                         ids=["label-too-large", "label-negative", "a-equals-b", "a-above-b"])
def test_bad_edges_are_refused(tn, vgs, rows, K):
    with pytest.raises(vgs.VgsError, match="VGS_E_ARG"):
        tn.fold_edges([_table([(0, 1, 1, 1, 1, 1, 0.5, 0.5, 0.5)]), _table(rows)], K)


@pytest.mark.parametrize("order", [[(1, 2), (0, 3)], [(0, 3), (0, 3)], [(0, 3), (0, 2)]], ids=["a-descends", "repeated", "b-descends"])
def test_an_unsorted_rank_table_is_refused(tn, vgs, order):
    t = _table([(0, 1, 1, 1, 1, 1, 0.5, 0.5, 0.5), (0, 2, 1, 1, 1, 1, 0.5, 0.5, 0.5)])
    bad = _table([(0, 1, 1, 1, 1, 1, 0.5, 0.5, 0.5), (0, 2, 1, 1, 1, 1, 0.5, 0.5, 0.5)])
    bad["seg_ab"] = np.array(order, dtype=np.int32)
    with pytest.raises(vgs.VgsError, match="VGS_E_ARG"):
        tn.fold_edges([t, bad], 10)
