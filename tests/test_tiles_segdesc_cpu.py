"""CPU tests of the descriptor fold of the tiled driver (vgs_tiles_fold_moments, csrc/tiles.cpp): per-rank moment records as
vgs_get_own_segment_moments gives them, some without own points, anchors 10^5 m from the origin.  The fold equals a numpy restatement of
its formulas (include/vgs_tiles.h), and the moments it folds give the centroid and covariance of the points behind them."""
import numpy as np
import pytest

PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


@pytest.fixture(scope="module")
def tn(vgs):
    from vgs_svgs_segmentation_amd import tiles_native
    tiles_native.lib()
    return tiles_native


def _rank_moments(pts, lab, K):
    """what one rank's kernels compute, in numpy: per label its points' count, float box, first point as anchor, fp64 sums about it"""
    rec = {"label": [], "n_points": [], "n_nodes": [], "bbox6": [], "anchor3": [], "s9": []}
    for k in range(K):
        p = pts[lab == k]
        if p.shape[0] == 0:
            continue
        a = p[0]
        d = p.astype(np.float64) - a.astype(np.float64)
        rec["label"].append(k)
        rec["n_points"].append(p.shape[0])
        rec["n_nodes"].append(1 + p.shape[0] // 7)
        rec["bbox6"].append(np.concatenate([p.min(axis=0), p.max(axis=0)]))
        rec["anchor3"].append(a)
        rec["s9"].append(np.concatenate([d.sum(axis=0), [(d[:, i] * d[:, j]).sum() for i, j in PAIRS]]))
    return _pack(rec)


def _pack(rec):
    n = len(rec["label"])
    return {"label": np.array(rec["label"], dtype=np.int32), "n_points": np.array(rec["n_points"], dtype=np.int64),
            "n_nodes": np.array(rec["n_nodes"], dtype=np.int32), "bbox6": np.array(rec["bbox6"], dtype=np.float32).reshape(n, 6),
            "anchor3": np.array(rec["anchor3"], dtype=np.float32).reshape(n, 3), "s9": np.array(rec["s9"], dtype=np.float64).reshape(n, 9)}


def _numpy_fold(records, K):
    """the fold of include/vgs_tiles.h restated: per label, ranks in ascending order"""
    n = np.zeros(K, np.int64)
    nn = np.zeros(K, np.int32)
    bb = np.tile(np.array([np.inf] * 3 + [-np.inf] * 3, np.float32), (K, 1))
    an = np.zeros((K, 3), np.float32)
    S = np.zeros((K, 9))
    for R in records:
        for i, k in enumerate(R["label"]):
            nn[k] += R["n_nodes"][i]
            bb[k, :3] = np.minimum(bb[k, :3], R["bbox6"][i, :3])
            bb[k, 3:] = np.maximum(bb[k, 3:], R["bbox6"][i, 3:])
            nr = R["n_points"][i]
            if nr <= 0:
                continue
            s = R["s9"][i]
            if n[k] == 0:
                an[k] = R["anchor3"][i]
                S[k] = s
            else:
                d = R["anchor3"][i].astype(np.float64) - an[k].astype(np.float64)
                S[k, :3] += s[:3] + nr * d
                for f, (a, b) in enumerate(PAIRS):
                    S[k, 3 + f] += s[3 + f] + s[a] * d[b] + d[a] * s[b] + nr * d[a] * d[b]
            n[k] += nr
    return dict(n_points=n, n_nodes=nn, bbox6=bb, anchor3=an, s9=S)


def _random_case(rng, world, K, origin):
    """K segments spread over `world` ranks; every rank sees only some of them; a few records hold owned voxels but no own point"""
    pts_all, lab_all, records = [], [], []
    for r in range(world):
        m = int(rng.integers(50, 400))
        seen = rng.choice(K, size=int(0.6 * K), replace=False)
        lab = seen[rng.integers(0, seen.size, size=m)]
        centre = origin + rng.normal(0, 20.0, size=(K, 3))
        p = (centre[lab] + rng.normal(0, rng.uniform(0.05, 3.0), size=(lab.size, 3))).astype(np.float32)
        R = _rank_moments(p, lab, K)
        # owned voxels whose points another rank loaded: records with n_points = 0
        extra = np.setdiff1d(rng.choice(K, size=K // 4, replace=False), R["label"])
        if extra.size:
            z = {"label": extra.astype(np.int32), "n_points": np.zeros(extra.size, np.int64),
                 "n_nodes": rng.integers(1, 4, size=extra.size).astype(np.int32),
                 "bbox6": np.tile(np.array([np.inf] * 3 + [-np.inf] * 3, np.float32), (extra.size, 1)),
                 "anchor3": np.zeros((extra.size, 3), np.float32), "s9": np.zeros((extra.size, 9))}
            order = np.argsort(np.concatenate([R["label"], z["label"]]), kind="stable")
            R = {f: np.concatenate([R[f], z[f]])[order] for f in R}
        records.append(R)
        pts_all.append(p)
        lab_all.append(lab)
    return records, np.concatenate(pts_all), np.concatenate(lab_all)


@pytest.mark.parametrize("world,seed", [(2, 1), (4, 2), (8, 3), (3, 4)])
def test_fold_equals_numpy_restatement(tn, world, seed):
    rng = np.random.default_rng(seed)
    K = 40
    records, _, _ = _random_case(rng, world, K, origin=np.array([1e5, -1e5, 30.0]))
    assert any((R["n_points"] == 0).any() for R in records)
    got = tn.fold_moments(records, K)
    ref = _numpy_fold(records, K)
    for f in ("n_points", "n_nodes", "bbox6", "anchor3"):
        assert np.array_equal(got[f], ref[f]), f
    np.testing.assert_allclose(got["s9"], ref["s9"], rtol=1e-13, atol=1e-9)
    # the anchor is the lowest rank's with own points
    for k in range(K):
        first = next((R["anchor3"][i] for R in records for i in np.flatnonzero(R["label"] == k) if R["n_points"][i] > 0), np.zeros(3, np.float32))
        assert np.array_equal(got["anchor3"][k], first)


@pytest.mark.parametrize("world,seed", [(2, 5), (4, 6), (8, 7)])
def test_folded_moments_give_the_points_moments(tn, world, seed):
    """the moments of every rank moved to one anchor: centroid and population covariance equal a two-pass numpy over all points"""
    rng = np.random.default_rng(seed)
    K = 30
    records, pts, lab = _random_case(rng, world, K, origin=np.array([-1e5, 1e5, 50.0]))
    got = tn.fold_moments(records, K)
    n = np.bincount(lab, minlength=K)
    assert np.array_equal(got["n_points"], n)
    live = n > 0
    x = pts.astype(np.float64)
    mean = np.stack([np.bincount(lab, x[:, a], minlength=K) for a in range(3)], axis=1) / np.maximum(n, 1)[:, None]
    mean += np.stack([np.bincount(lab, x[:, a] - mean[lab, a], minlength=K) for a in range(3)], axis=1) / np.maximum(n, 1)[:, None]
    d = x - mean[lab]
    cov = np.stack([np.bincount(lab, d[:, i] * d[:, j], minlength=K) for i, j in PAIRS], axis=1) / np.maximum(n, 1)[:, None]
    S, a = got["s9"], got["anchor3"].astype(np.float64)
    md = S[:, :3] / np.maximum(n, 1)[:, None]
    cen = a + md
    cv = np.stack([S[:, 3 + f] / np.maximum(n, 1) - md[:, i] * md[:, j] for f, (i, j) in enumerate(PAIRS)], axis=1)
    assert (np.abs(cen - mean)[live] <= 1e-9 * (1 + np.linalg.norm(mean, axis=1))[live, None]).all()
    tr = cov[:, [0, 3, 5]].sum(axis=1)
    assert (np.abs(cv - cov)[live] <= 1e-8 * tr[live, None] + 1e-12).all()
    lo = np.full((K, 3), np.inf, np.float32)
    hi = np.full((K, 3), -np.inf, np.float32)
    np.minimum.at(lo, lab, pts)
    np.maximum.at(hi, lab, pts)
    assert np.array_equal(got["bbox6"], np.concatenate([lo, hi], axis=1))


def test_fold_of_one_rank_is_its_records(tn):
    rng = np.random.default_rng(9)
    records, _, _ = _random_case(rng, 1, 25, origin=np.array([1e5, 1e5, 0.0]))
    got = tn.fold_moments(records, 25)
    R = records[0]
    own = R["n_points"] > 0
    assert np.array_equal(got["s9"][R["label"][own]].view(np.uint64), R["s9"][own].view(np.uint64))
    assert np.array_equal(got["anchor3"][R["label"][own]], R["anchor3"][own])


def test_fold_refuses_a_label_out_of_range(tn, vgs):
    rng = np.random.default_rng(10)
    records, _, _ = _random_case(rng, 2, 12, origin=np.zeros(3))
    with pytest.raises(vgs.VgsError):
        tn.fold_moments(records, 5)
