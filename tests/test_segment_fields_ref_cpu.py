"""tests/segment_fields_ref.py against a per-segment brute force on a random labelling: means and variances through math.fsum, counts,
min and max exactly.  The input holds NaN and +-inf, a segment whose values are all invalid, an empty label and unlabelled points."""
import math

import numpy as np

from segment_fields_ref import ref_class_hist, ref_field_stats

N, K, C = 4000, 9, 3
EMPTY, ALL_BAD = 4, 6   # a label no point carries; a segment whose channel 1 is invalid throughout


def _input():
    rng = np.random.default_rng(7)
    labels = rng.integers(-1, K, N).astype(np.int32)
    labels[labels == EMPTY] = -1
    field = (rng.normal(0.0, 3.0, (N, C)) + np.array([0.0, 1e4, -50.0])).astype(np.float32)
    bad = rng.choice(N * C, 300, replace=False)
    field.reshape(-1)[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), bad.size)
    field[labels == ALL_BAD, 1] = np.nan
    return field, labels


def test_field_stats_against_brute_force():
    field, labels = _input()
    anchor = np.zeros((K, C))
    for k in range(K):
        idx = np.nonzero(labels == k)[0]
        if idx.size:
            a = field[idx[0]].astype(np.float64)
            anchor[k] = np.where(np.isfinite(a), a, 0.0)
    r = ref_field_stats(field, labels, K, anchor)
    for k in range(K):
        for c in range(C):
            v = [float(x) for x in field[labels == k, c] if math.isfinite(x)]
            assert r["n_valid"][k, c] == len(v)
            if not v:
                assert all(math.isnan(r[f][k, c]) for f in ("mean", "var", "vmin", "vmax")), (k, c)
                continue
            assert r["vmin"][k, c] == np.float32(min(v)) and r["vmax"][k, c] == np.float32(max(v))
            n = len(v)
            mean = math.fsum(v) / n
            var = math.fsum((x - mean) ** 2 for x in v) / n
            # float64 sums of n terms about a point of the segment: relative error far below these bars
            assert abs(r["mean"][k, c] - mean) <= 1e-12 * (1 + abs(mean)), (k, c)
            assert abs(r["var"][k, c] - var) <= 1e-10 * (1 + var), (k, c)
    assert r["n_valid"][EMPTY].sum() == 0 and r["n_valid"][ALL_BAD, 1] == 0 and r["n_valid"][ALL_BAD, 0] > 0
    # a 1-d field is one channel
    r1 = ref_field_stats(field[:, 0], labels, K, anchor[:, :1])
    assert np.array_equal(r1["mean"], r["mean"][:, :1], equal_nan=True) and r1["n_valid"].shape == (K, 1)


def test_class_hist_against_brute_force():
    _, labels = _input()
    rng = np.random.default_rng(8)
    for n_classes in (1, 5):
        cls = rng.integers(-2, n_classes + 2, N).astype(np.int32)
        cls[:3] = np.iinfo(np.int32).max
        cls[labels == 2] = -1                      # every class outside: no majority
        tie = np.nonzero(labels == 3)[0]           # a constructed tie between the two highest classes
        if n_classes > 1:
            cls[tie] = np.where(np.arange(tie.size) % 2 == 0, n_classes - 1, n_classes - 2)
            cls[tie[-1]] = -1 if tie.size % 2 else cls[tie[-1]]
        r = ref_class_hist(cls, labels, K, n_classes)
        for k in range(K):
            mine = cls[labels == k].tolist()
            h = [sum(1 for v in mine if v == j) for j in range(n_classes)]
            assert r["hist"][k].tolist() == h
            assert r["n_outside"][k] == sum(1 for v in mine if v < 0 or v >= n_classes)
            best = max(h)
            assert r["majority_count"][k] == best
            assert r["majority"][k] == (h.index(best) if best > 0 else -1)
        assert r["majority"][2] == -1 and r["majority"][EMPTY] == -1 and r["hist"][EMPTY].sum() == 0
        if n_classes > 1:
            assert r["hist"][3, n_classes - 1] == r["hist"][3, n_classes - 2] > 0 and r["majority"][3] == n_classes - 2
