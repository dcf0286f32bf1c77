"""CPU tests of the extent fold of the tiled driver (vgs_tiles_fold_extents, csrc/tiles.cpp): per-rank extent records as
vgs_get_own_segment_extents gives them -- compact, ascending in label, a label on one rank, on several or on none.  The fold equals a
numpy restatement (include/vgs_tiles.h): per label the smallest lo and the largest hi over the ranks, `reached` where a record names the
label, +inf / -inf where none does.  Min and max return one of their inputs, so everything compares by value without a tolerance; a zero
bound may carry either sign."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def tn(vgs):
    from vgs_svgs_segmentation_amd import tiles_native
    tiles_native.lib()
    return tiles_native


def _rec(label, lo, hi):
    n = len(label)
    return {"label": np.array(label, dtype=np.int32), "lo3": np.array(lo, dtype=np.float64).reshape(n, 3),
            "hi3": np.array(hi, dtype=np.float64).reshape(n, 3)}


def _numpy_fold(records, K):
    lo = np.full((K, 3), np.inf)
    hi = np.full((K, 3), -np.inf)
    reached = np.zeros(K, np.uint8)
    for R in records:
        np.minimum.at(lo, R["label"], R["lo3"])
        np.maximum.at(hi, R["label"], R["hi3"])
        reached[R["label"]] = 1
    return lo, hi, reached


def _random_case(rng, world, K, empty=()):
    """labels 0 .. K-1: a third on exactly one rank, a third on several, a third on none; the ranks in `empty` send nothing"""
    live = [r for r in range(world) if r not in empty]
    where = {}
    for k in range(K):
        if k % 3 == 0:
            where[k] = [live[int(rng.integers(len(live)))]]
        elif k % 3 == 1:
            where[k] = sorted(rng.choice(live, size=min(len(live), int(rng.integers(2, 5))), replace=False).tolist())
        else:
            where[k] = []
    records = []
    for r in range(world):
        lab = [k for k in range(K) if r in where[k]]
        mid = rng.normal(0.0, 30.0, size=(len(lab), 3))
        ext = rng.uniform(0.0, 5.0, size=(len(lab), 3))
        ext[rng.random(len(lab)) < 0.2] = 0.0     # a one-point record: lo = hi
        records.append(_rec(lab, mid - ext, mid + ext))
    return records, where


@pytest.mark.parametrize("world,seed,empty", [(1, 1, ()), (3, 2, ()), (8, 3, ()), (3, 4, (1,)), (8, 5, (0, 7))],
                         ids=["w1", "w3", "w8", "w3_empty_rank", "w8_empty_ranks"])
def test_fold_equals_numpy_restatement(tn, world, seed, empty):
    rng = np.random.default_rng(seed)
    K = 60
    records, where = _random_case(rng, world, K, empty)
    for r in empty:
        assert records[r]["label"].size == 0
    n_ranks = np.array([len(where[k]) for k in range(K)])
    assert (n_ranks == 0).any() and (n_ranks == 1).any() and (world == 1 or (n_ranks >= 2).any())
    got = tn.fold_extents(records, K)
    lo, hi, reached = _numpy_fold(records, K)
    assert got["lo3"].shape == (K, 3) and got["hi3"].shape == (K, 3) and got["reached"].shape == (K,)
    assert np.array_equal(got["reached"], reached) and np.array_equal(reached, (n_ranks > 0).astype(np.uint8))
    assert (got["lo3"] == lo).all() and (got["hi3"] == hi).all()
    none = reached == 0
    assert (got["lo3"][none] == np.inf).all() and (got["hi3"][none] == -np.inf).all()
    assert (got["lo3"][~none] <= got["hi3"][~none]).all()


def test_fold_of_one_rank_is_its_records(tn):
    rng = np.random.default_rng(9)
    records, _ = _random_case(rng, 1, 30)
    got = tn.fold_extents(records, 30)
    R = records[0]
    assert np.array_equal(got["lo3"][R["label"]].view(np.uint64), R["lo3"].view(np.uint64))
    assert np.array_equal(got["hi3"][R["label"]].view(np.uint64), R["hi3"].view(np.uint64))


def test_signed_zero_bounds_compare_by_value(tn):
    """-0.0 on one rank against +0.0 on another, in either order: the bound is a zero (whichever sign), never the other rank's non-zero"""
    a = _rec([0, 1], [[-0.0, 0.0, -1.0], [0.0, -0.0, -2.0]], [[0.0, -0.0, 1.0], [-0.0, 0.0, 3.0]])
    b = _rec([0, 1], [[0.0, -0.0, 0.5], [-0.0, 0.0, 0.0]], [[-0.0, 0.0, 0.5], [0.0, -0.0, -0.0]])
    for records in ([a, b], [b, a], [a, _rec([], [], []), b]):
        got = tn.fold_extents(records, 2)
        assert (got["lo3"] == np.array([[0.0, 0.0, -1.0], [0.0, 0.0, -2.0]])).all()
        assert (got["hi3"] == np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 3.0]])).all()
        assert got["reached"].tolist() == [1, 1]
        lo, hi, _ = _numpy_fold(records, 2)
        assert (got["lo3"] == lo).all() and (got["hi3"] == hi).all()


def test_no_segments_and_no_records(tn):
    empty = _rec([], [], [])
    got = tn.fold_extents([empty, empty, empty], 0)
    assert got["lo3"].shape == (0, 3) and got["hi3"].shape == (0, 3) and got["reached"].shape == (0,)
    got = tn.fold_extents([empty, empty], 4)
    assert (got["lo3"] == np.inf).all() and (got["hi3"] == -np.inf).all() and (got["reached"] == 0).all()


@pytest.mark.parametrize("bad", [5, 6, -1], ids=["label_eq_K", "label_gt_K", "negative"])
def test_fold_refuses_a_label_out_of_range(tn, vgs, bad):
    ok = _rec([0, 4], [[0, 0, 0], [1, 1, 1]], [[1, 1, 1], [2, 2, 2]])
    assert tn.fold_extents([ok, ok], 5)["reached"].tolist() == [1, 0, 0, 0, 1]
    wrong = _rec([0, bad] if bad > 0 else [bad, 0], [[0, 0, 0], [1, 1, 1]], [[1, 1, 1], [2, 2, 2]])
    with pytest.raises(vgs.VgsError) as e:
        tn.fold_extents([ok, wrong], 5)
    assert e.value.status == vgs._lib.VGS_E_ARG
    with pytest.raises(vgs.VgsError) as e:
        tn.fold_extents([wrong], 5)
    assert e.value.status == vgs._lib.VGS_E_ARG
