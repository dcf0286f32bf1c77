"""CPU tests of the two attribute folds of the tiled driver (vgs_tiles_fold_field_moments, vgs_tiles_fold_class_counts, csrc/tiles.cpp) on
the case generator of test_tiles_segbox_cpu.py: per-rank records as vgs_get_own_segment_field_moments / vgs_get_own_segment_class_counts
give them -- compact, ascending in label, a label on one rank, on several or on none, ranks that send nothing.  Each fold equals a numpy
restatement of include/vgs_tiles.h taken rank by rank in the header's association: counts, min, max, the anchor and the histogram by
value; S1 and S2 by value for integer-valued records (every term an exact integer below 2^53) and to rtol 1e-13 for general ones (the
bar of test_tiles_segdesc_cpu.py: the restatement's own operations are numpy's)."""
import numpy as np
import pytest

from test_tiles_segbox_cpu import _random_case

FM = ("n_valid", "anchor", "s1", "s2", "vmin", "vmax")


@pytest.fixture(scope="module")
def tn(vgs):
    from vgs_svgs_segmentation_amd import tiles_native
    tiles_native.lib()
    return tiles_native


def _field_records(rng, world, K, C, empty=(), integer=False):
    """moment records over the labels of _random_case: n points per (record, channel) drawn about an anchor that is one of them; a fifth of
    the entries hold no valid value (n 0, anchor and sums 0, +inf / -inf)"""
    boxes, where = _random_case(rng, world, K, empty)
    records = []
    for r in range(world):
        lab = boxes[r]["label"]
        m = lab.size
        R = {"label": lab, "n_valid": np.zeros((m, C), np.int64), "anchor": np.zeros((m, C)), "s1": np.zeros((m, C)), "s2": np.zeros((m, C)),
             "vmin": np.full((m, C), np.inf, np.float32), "vmax": np.full((m, C), -np.inf, np.float32)}
        for i in range(m):
            for c in range(C):
                if rng.random() < 0.2:
                    continue
                n = int(rng.integers(1, 40))
                x = (rng.integers(0, 4096, n) if integer else rng.normal(1e4 * c, 3.0, n)).astype(np.float32)
                a = float(x[0]) if rng.random() < 0.8 else 0.0        # (an anchor that met an invalid value is 0.0)
                d = x.astype(np.float64) - a
                R["n_valid"][i, c], R["anchor"][i, c], R["s1"][i, c], R["s2"][i, c] = n, a, d.sum(), (d * d).sum()
                R["vmin"][i, c], R["vmax"][i, c] = x.min(), x.max()
        records.append(R)
    return records, where


def _numpy_fold_moments(records, K, C):
    n = np.zeros((K, C), np.int64)
    a, s1, s2 = np.zeros((K, C)), np.zeros((K, C)), np.zeros((K, C))
    mn, mx = np.full((K, C), np.inf, np.float32), np.full((K, C), -np.inf, np.float32)
    for R in records:
        for i, k in enumerate(R["label"].tolist()):
            for c in range(C):
                mn[k, c], mx[k, c] = min(mn[k, c], R["vmin"][i, c]), max(mx[k, c], R["vmax"][i, c])
                nr = int(R["n_valid"][i, c])
                if nr == 0:
                    continue
                if n[k, c] == 0:
                    n[k, c], a[k, c], s1[k, c], s2[k, c] = nr, R["anchor"][i, c], R["s1"][i, c], R["s2"][i, c]
                    continue
                d = R["anchor"][i, c] - a[k, c]
                s1r = R["s1"][i, c]
                s1[k, c] += s1r + nr * d
                s2[k, c] += R["s2"][i, c] + s1r * d + d * s1r + nr * d * d
                n[k, c] += nr
    return dict(n_valid=n, anchor=a, s1=s1, s2=s2, vmin=mn, vmax=mx)


CASES = [(1, 1, ()), (3, 2, ()), (8, 3, ()), (3, 4, (1,)), (8, 5, (0, 7))]
IDS = ["w1", "w3", "w8", "w3_empty_rank", "w8_empty_ranks"]


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "general"])
@pytest.mark.parametrize("world,seed,empty", CASES, ids=IDS)
def test_moment_fold_equals_numpy_restatement(tn, world, seed, empty, integer):
    rng = np.random.default_rng(seed)
    K, C = 60, 3
    records, where = _field_records(rng, world, K, C, empty, integer)
    for r in empty:
        assert records[r]["label"].size == 0
    n_ranks = np.array([len(where[k]) for k in range(K)])
    assert (n_ranks == 0).any() and (n_ranks == 1).any() and (world == 1 or (n_ranks >= 2).any())
    got = tn.fold_field_moments(records, K, C)
    ref = _numpy_fold_moments(records, K, C)
    assert all(got[f].shape == (K, C) for f in FM)
    for f in ("n_valid", "anchor", "vmin", "vmax"):
        assert np.array_equal(got[f], ref[f]), f
    if integer:
        assert np.abs(ref["s2"]).max() < 2.0 ** 53
        assert np.array_equal(got["s1"], ref["s1"]) and np.array_equal(got["s2"], ref["s2"])
        # and the integers are the right ones: the moments of the union about the folded anchor, whatever each rank's own anchor was
        assert (got["s1"] == np.rint(got["s1"])).all()
    else:
        np.testing.assert_allclose(got["s1"], ref["s1"], rtol=1e-13, atol=1e-9)
        np.testing.assert_allclose(got["s2"], ref["s2"], rtol=1e-13, atol=1e-9)
    none = got["n_valid"] == 0
    assert none.any() and (got["anchor"][none] == 0).all() and (got["s1"][none] == 0).all() and (got["s2"][none] == 0).all()
    assert (got["vmin"][none] == np.inf).all() and (got["vmax"][none] == -np.inf).all()
    assert (got["vmin"][~none] <= got["vmax"][~none]).all()


def test_integer_moments_are_those_of_the_union(tn):
    """two ranks with the values in hand: the folded sums are the sums of all values about rank 0's anchor, exactly"""
    x0, x1 = np.array([7, 100, 4095], np.float64), np.array([0, 3000, 12, 900], np.float64)
    r0 = {"label": np.array([2], np.int32), "n_valid": [[3]], "anchor": [[7.0]], "s1": [[(x0 - 7).sum()]], "s2": [[((x0 - 7) ** 2).sum()]],
          "vmin": [[7]], "vmax": [[4095]]}
    r1 = {"label": np.array([2], np.int32), "n_valid": [[4]], "anchor": [[3000.0]], "s1": [[(x1 - 3000).sum()]], "s2": [[((x1 - 3000) ** 2).sum()]],
          "vmin": [[0]], "vmax": [[3000]]}
    got = tn.fold_field_moments([r0, r1], 3, 1)
    x = np.concatenate([x0, x1])
    assert got["n_valid"][2, 0] == 7 and got["anchor"][2, 0] == 7.0
    assert got["s1"][2, 0] == (x - 7).sum() and got["s2"][2, 0] == ((x - 7) ** 2).sum()
    assert got["vmin"][2, 0] == 0 and got["vmax"][2, 0] == 4095
    assert (got["n_valid"][[0, 1]] == 0).all()


def test_anchor_is_the_lowest_rank_with_a_valid_value(tn):
    """rank 0 names the label but has n_valid = 0 (its anchor is 0.0 and must not be taken): the anchor is rank 1's, whose sums pass as they
    are; rank 2 is shifted onto it"""
    def rec(n, a, s1, s2, lo, hi):
        return {"label": np.array([0], np.int32), "n_valid": [[n]], "anchor": [[a]], "s1": [[s1]], "s2": [[s2]], "vmin": [[lo]], "vmax": [[hi]]}
    r0 = rec(0, 0.0, 0.0, 0.0, np.inf, -np.inf)
    r1 = rec(2, 10.0, 4.0, 10.0, 11.0, 13.0)          # values 11, 13 about 10
    r2 = rec(1, 20.0, 0.0, 0.0, 20.0, 20.0)           # value 20 about 20
    got = tn.fold_field_moments([r0, r1, r2], 1, 1)
    assert got["anchor"][0, 0] == 10.0 and got["n_valid"][0, 0] == 3
    assert got["s1"][0, 0] == 1 + 3 + 10 and got["s2"][0, 0] == 1 + 9 + 100
    assert got["vmin"][0, 0] == 11.0 and got["vmax"][0, 0] == 20.0
    only = tn.fold_field_moments([r0, r1], 1, 1)
    assert only["anchor"][0, 0] == 10.0 and only["s1"][0, 0] == 4.0 and only["s2"][0, 0] == 10.0 and only["n_valid"][0, 0] == 2
    nobody = tn.fold_field_moments([r0, r0], 1, 1)
    assert nobody["n_valid"][0, 0] == 0 and nobody["anchor"][0, 0] == 0 and nobody["vmin"][0, 0] == np.inf and nobody["vmax"][0, 0] == -np.inf


def test_a_single_record_passes_through_bit_for_bit(tn):
    rng = np.random.default_rng(11)
    records, _ = _field_records(rng, 1, 30, 5)
    R = records[0]
    got = tn.fold_field_moments(records, 30, 5)
    valid = R["n_valid"] > 0
    for f in FM:
        a, b = got[f][R["label"]], np.asarray(R[f], dtype=got[f].dtype)
        assert np.array_equal(a[valid].view(np.uint8), b[valid].view(np.uint8)), f
    # the same record behind ranks that send nothing
    empty = {k: np.asarray(v)[:0] for k, v in R.items()}
    again = tn.fold_field_moments([empty, R, empty], 30, 5)
    assert all(np.array_equal(again[f].view(np.uint8), got[f].view(np.uint8)) for f in FM)
    # class counts
    C = {"label": np.array([1, 4], np.int32), "hist": np.array([[0, 5, 5], [2, 0, 0]], np.int64), "n_outside": np.array([3, 0], np.int64)}
    h = tn.fold_class_counts([C], 5, 3)
    assert np.array_equal(h["hist"][[1, 4]], C["hist"]) and np.array_equal(h["n_outside"][[1, 4]], C["n_outside"])
    assert h["majority"].tolist() == [-1, 1, -1, -1, 0] and h["majority_count"].tolist() == [0, 5, 0, 0, 2]      # a tie: the lower class


def _class_records(rng, world, K, nc, empty=()):
    boxes, where = _random_case(rng, world, K, empty)
    records = []
    for r in range(world):
        lab = boxes[r]["label"]
        hist = rng.integers(0, 50, (lab.size, nc)).astype(np.int64)
        hist[rng.random(lab.size) < 0.2] = 0                      # every class outside
        records.append({"label": lab, "hist": hist, "n_outside": rng.integers(0, 9, lab.size).astype(np.int64)})
    return records, where


@pytest.mark.parametrize("nc", [1, 16, 1024])
@pytest.mark.parametrize("world,seed,empty", CASES, ids=IDS)
def test_class_fold_equals_numpy_restatement(tn, world, seed, empty, nc):
    rng = np.random.default_rng(100 + seed)
    K = 60
    records, where = _class_records(rng, world, K, nc, empty)
    hist, nout = np.zeros((K, nc), np.int64), np.zeros(K, np.int64)
    for R in records:
        np.add.at(hist, R["label"], R["hist"])
        np.add.at(nout, R["label"], R["n_outside"])
    best = hist.max(axis=1)
    got = tn.fold_class_counts(records, K, nc)
    assert [got[k].dtype for k in ("hist", "n_outside", "majority", "majority_count")] == [np.int64, np.int64, np.int32, np.int64]
    assert np.array_equal(got["hist"], hist) and np.array_equal(got["n_outside"], nout)
    assert np.array_equal(got["majority_count"], best)
    assert np.array_equal(got["majority"], np.where(best > 0, hist.argmax(axis=1), -1))      # argmax: the lowest index on a tie
    assert (got["majority"] == -1).any()


def test_no_segments_and_no_records(tn):
    e = {"label": np.zeros(0, np.int32), **{f: np.zeros((0, 2)) for f in FM}}
    got = tn.fold_field_moments([e, e, e], 0, 2)
    assert all(got[f].shape == (0, 2) for f in FM)
    got = tn.fold_field_moments([e, e], 4, 2)
    assert (got["n_valid"] == 0).all() and (got["vmin"] == np.inf).all() and (got["vmax"] == -np.inf).all()
    c = {"label": np.zeros(0, np.int32), "hist": np.zeros((0, 3), np.int64), "n_outside": np.zeros(0, np.int64)}
    h = tn.fold_class_counts([c, c], 4, 3)
    assert (h["hist"] == 0).all() and (h["majority"] == -1).all() and (h["majority_count"] == 0).all()
    assert tn.fold_class_counts([c], 0, 3)["hist"].shape == (0, 3)


@pytest.mark.parametrize("bad", [5, 6, -1], ids=["label_eq_K", "label_gt_K", "negative"])
def test_folds_refuse_a_label_out_of_range(tn, vgs, bad):
    def frec(labels):
        m = len(labels)
        return {"label": np.array(labels, np.int32), "n_valid": np.ones((m, 2), np.int64), "anchor": np.zeros((m, 2)), "s1": np.zeros((m, 2)),
                "s2": np.zeros((m, 2)), "vmin": np.zeros((m, 2), np.float32), "vmax": np.zeros((m, 2), np.float32)}

    def crec(labels):
        return {"label": np.array(labels, np.int32), "hist": np.ones((len(labels), 3), np.int64), "n_outside": np.zeros(len(labels), np.int64)}
    labels = [0, bad] if bad > 0 else [bad, 0]
    assert tn.fold_field_moments([frec([0, 4]), frec([0, 4])], 5, 2)["n_valid"][:, 0].tolist() == [2, 0, 0, 0, 2]
    assert tn.fold_class_counts([crec([0, 4]), crec([0, 4])], 5, 3)["hist"][:, 0].tolist() == [2, 0, 0, 0, 2]
    for call in (lambda: tn.fold_field_moments([frec([0, 4]), frec(labels)], 5, 2), lambda: tn.fold_field_moments([frec(labels)], 5, 2),
                 lambda: tn.fold_class_counts([crec([0, 4]), crec(labels)], 5, 3), lambda: tn.fold_class_counts([crec(labels)], 5, 3)):
        with pytest.raises(vgs.VgsError) as e:
            call()
        assert e.value.status == vgs._lib.VGS_E_ARG
