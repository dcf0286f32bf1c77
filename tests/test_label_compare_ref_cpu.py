"""The numpy restatement of the label comparison (tests/label_compare_ref.py) against a brute-force double loop on small clouds, against
helpers.partition_agreement, and api.comparison_scores against the formulas written out independently.  No GPU."""
import math

import numpy as np
import pytest

import helpers
import label_compare_ref as R
import vgs_svgs_segmentation_amd as v

INT32_MAX = 2**31 - 1


def _cases():
    rng = np.random.default_rng(20)
    out = {}
    for i, (n, K, G) in enumerate(((200, 7, 5), (150, 3, 40), (97, 12, 3), (200, 1, 1), (64, 30, 30))):
        lab = rng.integers(-1, K, n).astype(np.int32)
        ref = rng.integers(-2, G, n).astype(np.int32) * 37   # sparse ids, a few negative
        out[f"random{i}"] = (lab, ref, K)
    # ties on both sides: segment 0 holds two points of id 5 and two of id 9 (the lower id wins); id 9 holds two points of segment 0 and
    # two of segment 2 (the lower label wins); segment 1 ties ids 3 and 5 with one point each
    out["ties"] = (np.array([0, 0, 0, 0, 2, 2, 1, 1, -1], np.int32), np.array([9, 5, 9, 5, 9, 9, 5, 3, 9], np.int32), 3)
    out["int32_max"] = (np.array([0, 0, 1, 1, 1, -1], np.int32), np.array([0, INT32_MAX, INT32_MAX, INT32_MAX, 0, INT32_MAX], np.int32), 2)
    out["all_unannotated"] = (rng.integers(-1, 4, 50).astype(np.int32), np.full(50, -7, np.int32), 4)
    out["all_dropped"] = (np.full(60, -1, np.int32), rng.integers(0, 5, 60).astype(np.int32), 3)
    out["k0"] = (np.full(40, -1, np.int32), rng.integers(-1, 6, 40).astype(np.int32), 0)
    out["single_id"] = (rng.integers(-1, 5, 120).astype(np.int32), np.full(120, 11, np.int32), 5)
    out["no_points"] = (np.zeros(0, np.int32), np.zeros(0, np.int32), 0)
    out["empty_segment"] = (np.array([0, 0, 3, 3, 3], np.int32), np.array([1, 2, 2, -1, 2], np.int32), 5)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_brute_force(name):
    lab, ref, K = CASES[name]
    assert lab.size <= 200
    a, b = R.compare_labels(lab, ref, K), R.compare_brute(lab, ref, K)
    assert R.same(a, b), R.diff(a, b)
    s = a["summary"]
    assert s[0] + s[1] == lab.size and s[3] == a["ref_id"].size and s[4] == a["cell_n"].size and a["seg_annotated"].size == K
    assert a["cell_n"].sum() == s[0] and a["ref_points"].sum() == s[0] and a["seg_annotated"].sum() + s[2] == s[0]


def test_expected_values_of_the_edge_cases():
    t = R.compare_labels(*CASES["ties"])
    assert t["seg_best_ref"].tolist() == [5, 3, 9] and t["seg_best_n"].tolist() == [2, 1, 2]
    assert t["ref_id"].tolist() == [3, 5, 9] and t["ref_best_seg"].tolist() == [1, 0, 0] and t["ref_dropped"].tolist() == [0, 0, 1]
    m = R.compare_labels(*CASES["int32_max"])
    assert m["ref_id"].tolist() == [0, INT32_MAX] and m["cell_ref"].max() == INT32_MAX and m["ref_best_seg"].tolist() == [0, 1]
    u = R.compare_labels(*CASES["all_unannotated"])
    assert u["summary"].tolist() == [0, 50] + [0] * 10 and u["cell_n"].size == 0 and u["ref_id"].size == 0
    assert u["seg_best_ref"].tolist() == [-1] * 4 and not u["seg_best_iou"].any() and not u["seg_annotated"].any()
    d = R.compare_labels(*CASES["all_dropped"])
    assert d["summary"][2] == 60 and (d["ref_best_seg"] == -1).all() and not d["ref_best_iou"].any() and (d["cell_seg"] == -1).all()
    assert np.array_equal(d["ref_dropped"], d["ref_points"])
    k0 = R.compare_labels(*CASES["k0"])
    assert k0["seg_annotated"].size == 0 and k0["summary"][5] == 0 and k0["summary"][6] == 0 and k0["summary"][7] == 0
    e = R.compare_labels(*CASES["no_points"])
    assert not e["summary"].any() and all(e[n].size == 0 for n, _ in R.FIELDS if n != "summary")


@pytest.mark.parametrize("seed", range(4))
def test_completeness_is_partition_agreement(seed):
    rng = np.random.default_rng(seed)
    n, K = 180, 9
    lab = rng.integers(0, K, n).astype(np.int32)          # no segment dropped
    ref = (rng.integers(0, 6, n) * 1000).astype(np.int32)   # every point annotated
    s = R.compare_labels(lab, ref, K)["summary"]
    assert s[7] / s[0] == helpers.partition_agreement(ref, lab)
    assert s[6] / s[0] == helpers.partition_agreement(lab, ref)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("tau", (0.5, 0.6, 0.75, 0.999))
def test_scores_against_the_formulas(name, tau):
    lab, ref, K = CASES[name]
    cmp = R.compare_labels(lab, ref, K)
    got, want = v.comparison_scores(cmp, tau), R.scores_formulas(cmp, tau)
    assert got["matched"] == want["matched"] and got["tau"] == tau
    for key in ("precision", "recall", "f1", "purity", "completeness", "ari"):
        assert R.close(got[key], want[key]), (key, got[key], want[key])


def test_scores_of_a_perfect_and_of_an_empty_comparison():
    lab = np.repeat(np.arange(5, dtype=np.int32), 7)
    s = v.comparison_scores(R.compare_labels(lab, lab * 3 + 1, 5))
    assert s == {"tau": 0.5, "matched": 5, "precision": 1.0, "recall": 1.0, "f1": 1.0, "purity": 1.0, "completeness": 1.0, "ari": 1.0}
    e = v.comparison_scores(R.compare_labels(*CASES["no_points"]))
    assert e["matched"] == 0 and all(math.isnan(e[k]) for k in ("precision", "recall", "f1", "purity", "completeness", "ari"))
    for tau in (0.49, 1.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="tau"):
            v.comparison_scores(R.compare_labels(lab, lab, 5), tau)


@pytest.mark.parametrize("name", sorted(CASES))
def test_matched_is_the_same_from_both_tables(name):
    """IoU > tau >= 0.5 makes segment and id each other's best match, so either table counts the same pairs"""
    cmp = R.compare_labels(*CASES[name])
    ious = np.concatenate([cmp["seg_best_iou"], cmp["ref_best_iou"], [0.5]])
    for tau in sorted(set(float(t) for t in ious if 0.5 <= t < 1.0) | {0.5, 0.75, 0.9}):
        assert int((cmp["seg_best_iou"] > tau).sum()) == int((cmp["ref_best_iou"] > tau).sum()), tau
