"""Field statistics and class histograms of a caller's per-POINT labelling (vgs_point_label_field_stats, vgs_point_label_class_histogram;
csrc/pointfield.hip): Engine.label_field_stats and label_class_histogram.

The main acceptance test: handed the engine's own point labels, the new pass returns segment_field_stats() and segment_class_histogram()
byte for byte, anchor included.  Then what the node pass cannot express -- labels that alternate inside voxels -- on integer-valued
fields, whose sums are exact in any order, against tests/segment_fields_ref.py evaluated at the engine's own anchor, by value and without
a tolerance; labels at the chunk and fold limits (SD_CHUNK = 2048 points per chunk, 64 partials per fold step), empty labels, K = 1 and
0; general floats against math.fsum within the summation bound of test_gpu_segment_fields.py; the anchor contract; invalid values; the
histogram's ties and all-outside rows; labelled points outside the octree; row permutation; the refined labels; determinism and input
forms; the status contract; and vgs_run's --refined-segment-fields / --refined-segment-classes.

The reference labelling of every check against the restatement is `labels` with the points outside the octree (point_voxel() < 0: the
non-finite points, for SVGS those of no supervoxel) set to -1."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import helpers
from label_refine_scenes import GROUP5, big_boundary_voxel, dropped_beside_kept
from segment_fields_ref import ref_class_hist, ref_field_stats
from segment_scenes import FAR, SPLIT, two_tilted_planes
from test_cpp_segment_desc import CSRC, RUN, VGS_LINES, _write_task

pytestmark = pytest.mark.gpu

SD_CHUNK = 2048   # points per chunk (csrc/vgs_context.hpp: SD_TB * SD_PPT)
STAT_KEYS = ("n_valid", "anchor", "mean", "var", "vmin", "vmax")
HIST_KEYS = ("hist", "n_outside", "majority", "majority_count")
U = 2.0 ** -52
_cache = {}


def _engine(gpu, xyz, method=2, **kw):
    eng = gpu.Engine(gpu.default_params(method, **kw))
    eng.set_points(xyz)
    eng.run()
    return eng


def _urban(gpu, method):
    """urban_scene(150 000) segmented by VGS or SVGS, made once and shared; the tests leave the engine segmented"""
    if ("urban", method) not in _cache:
        xyz = gpu.scenes.urban_scene(150_000)
        _cache["urban", method] = (xyz, _engine(gpu, xyz, method))
    return _cache["urban", method]


def _plain(gpu):
    if "plain" not in _cache:
        xyz = np.random.default_rng(77).uniform(0.0, 6.0, size=(200_000, 3)).astype(np.float32)
        _cache["plain"] = (xyz, _engine(gpu, xyz))
    return _cache["plain"]


def _diff(a, b, keys):
    """the keys whose arrays differ in dtype, shape or bytes"""
    return [k for k in keys if not (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes())]


def _int_field(n, ch, seed):
    return np.random.default_rng(seed).integers(0, 4096, (n, ch)).astype(np.float32)


def _classes(n, n_classes, seed):
    cls = np.random.default_rng(seed).integers(-1, n_classes + 1, n).astype(np.int32)   # -1 and n_classes included
    cls[::97] = np.iinfo(np.int32).max
    return cls


def _inside(eng, labels):
    """the reference labelling: labels with every point outside the octree set to -1; and the number of labelled points among those"""
    out = eng.point_voxel() < 0
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    return np.where(out, -1, labels).astype(np.int32), int(((labels >= 0) & out).sum())


def _check_exact(eng, labels, K, field, cls=None, n_classes=0):
    """label_field_stats (and label_class_histogram) of an arbitrary labelling against the restatement over the octree points: the field
    table at its own anchor, by value, for integer-valued fields whose d and d * d sum exactly; the histogram exactly; both against the
    point counts of describe_labels for the same labelling."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    lab_in, skipped = _inside(eng, labels)
    n_points = eng.describe_labels(labels, K=K)["n_points"]
    assert np.array_equal(n_points, np.bincount(lab_in[lab_in >= 0], minlength=K))
    got = eng.label_field_stats(labels, field, K=K)
    ch = 1 if field.ndim == 1 else field.shape[1]
    assert got["n_skipped"] == skipped
    assert all(got[k].shape == (K, ch) for k in STAT_KEYS)
    assert [got[k].dtype for k in STAT_KEYS] == [np.int64, np.float64, np.float64, np.float64, np.float32, np.float32]
    finite = field[np.isfinite(field)]
    assert (finite == np.rint(finite)).all() and np.abs(finite).max() <= 4095
    assert int(n_points.max(initial=0)) * 4095.0 ** 2 < 2.0 ** 53   # every partial sum of d (|d| <= 4095) and of d * d is an exact integer
    ref = ref_field_stats(field, lab_in, K, got["anchor"])
    for k in ("n_valid", "mean", "var", "vmin", "vmax"):
        g, r = got[k].astype(np.float64), ref[k].astype(np.float64)
        bad = np.nonzero(~((g == r) | (np.isnan(g) & np.isnan(r))))
        assert bad[0].size == 0, (k, bad[0][:5], bad[1][:5], got[k][bad][:5], ref[k][bad][:5])
    assert (got["n_valid"] <= n_points[:, None]).all()
    empty = n_points == 0
    assert (got["n_valid"][empty] == 0).all() and (got["anchor"][empty] == 0).all()
    assert all(np.isnan(got[k][empty]).all() for k in ("mean", "var", "vmin", "vmax"))
    hist = None
    if cls is not None:
        hist = eng.label_class_histogram(labels, cls, n_classes, K=K)
        assert hist["n_skipped"] == skipped
        assert [hist[k].dtype for k in HIST_KEYS] == [np.int64, np.int64, np.int32, np.int64]
        assert hist["hist"].shape == (K, n_classes) and all(hist[k].shape == (K,) for k in HIST_KEYS[1:])
        rh = ref_class_hist(cls, lab_in, K, n_classes)
        for k in HIST_KEYS:
            assert np.array_equal(hist[k], rh[k]), k
        assert np.array_equal(hist["hist"].sum(axis=1) + hist["n_outside"], n_points)
        assert (hist["majority"][empty] == -1).all() and (hist["majority_count"][empty] == 0).all()
    return got, hist, n_points


# ---------------------------------------------------------------- 1. byte equality with the node tables
@pytest.mark.parametrize("method", [2, 3], ids=["vgs", "svgs"])
def test_own_point_labels_reproduce_the_node_tables(gpu, method):
    xyz, eng = _urban(gpu, method)
    labels, K = eng.point_labels(), eng.counts()["kept"]
    N = xyz.shape[0]
    assert K > 10
    for ch in (1, 5, 64):   # (five channels: a ragged second group)
        field = np.random.default_rng(30 + ch).normal(100.0, 7.0, (N, ch)).astype(np.float32)
        field[::53, 0] = np.nan
        got, want = eng.label_field_stats(labels, field), eng.segment_field_stats(field)
        assert got.pop("n_skipped") == 0
        assert sorted(got) == sorted(want) and not _diff(got, want, STAT_KEYS), (ch, _diff(got, want, STAT_KEYS))
    for nc in (1, 7, 1024):
        cls = _classes(N, nc, 40 + nc)
        got, want = eng.label_class_histogram(labels, cls, nc), eng.segment_class_histogram(cls, nc)
        assert got.pop("n_skipped") == 0
        assert sorted(got) == sorted(want) and not _diff(got, want, HIST_KEYS), (nc, _diff(got, want, HIST_KEYS))


# ---------------------------------------------------------------- 2. labels that alternate inside voxels, near and far
def _mixed_scenes():
    a = big_boundary_voxel()
    la = (np.arange(a.shape[0]) % 3).astype(np.int32)
    b = two_tilted_planes()
    side = (b[:, 0] + 0.37 * b[:, 1] > 2.9).astype(np.int32)   # a plane that cuts through voxels
    lb = (np.arange(b.shape[0]) % 3 + 3 * side).astype(np.int32)
    return {"boundary_voxel": (a, la, 4, SPLIT), "tilted_planes": (b, lb, 7, {})}   # (the last label of either: no point)


@pytest.mark.parametrize("name", ["boundary_voxel", "tilted_planes"])
@pytest.mark.parametrize("far", [False, True], ids=["near", "far"])
def test_labels_that_alternate_inside_voxels(gpu, name, far):
    xyz, labels, K, kw = _mixed_scenes()[name]
    if far:
        xyz = (xyz.astype(np.float64) + np.array(FAR)).astype(np.float32)
    eng = _engine(gpu, xyz, **kw)
    pv = eng.point_voxel()
    per_voxel = np.unique(np.stack([pv.astype(np.int64), labels.astype(np.int64)], axis=1), axis=0)
    assert np.bincount(per_voxel[:, 0]).max() >= 3   # single nodes hold three labels: no labelling of nodes says this
    N = xyz.shape[0]
    got, hist, n_points = _check_exact(eng, labels, K, _int_field(N, 5, 51), _classes(N, 7, 52), 7)
    assert (n_points[:3] > 0).all() and n_points[K - 1] == 0


# ---------------------------------------------------------------- 3. chunk and fold limits
def test_chunk_and_fold_limits(gpu):
    xyz, eng = _plain(gpu)
    N = xyz.shape[0]
    field, cls = _int_field(N, 5, 53), _classes(N, 7, 54)
    sizes = {0: 1, 2: SD_CHUNK - 1, 3: SD_CHUNK, 6: SD_CHUNK + 1, 7: 140_000}   # 140 000 > 64 * SD_CHUNK: the lane-stride fold wraps
    K = 9                                                                         # labels 1, 4, 5 and the last one, 8: no point
    assert sizes[7] > 64 * SD_CHUNK
    labels = np.full(N, -1, np.int32)
    at = 11
    for k, n in sizes.items():
        labels[at:at + n] = k
        at += n + 5
    got, hist, n_points = _check_exact(eng, labels, K, field, cls, 7)
    assert n_points.tolist() == [1, 0, SD_CHUNK - 1, SD_CHUNK, 0, 0, SD_CHUNK + 1, 140_000, 0]
    assert np.array_equal(got["n_valid"], np.repeat(n_points[:, None], 5, axis=1))
    # K = 1: everything one label; and one label of under a chunk
    _check_exact(eng, np.zeros(N, np.int32), 1, field, cls, 7)
    one = np.full(N, -1, np.int32)
    one[5:900] = 0
    _check_exact(eng, one, 1, field[:, 0].copy(), cls, 7)
    # every label negative: all rows empty
    got, hist, n_points = _check_exact(eng, np.full(N, -7, np.int32), 4, field, cls, 7)
    assert not n_points.any() and not got["n_valid"].any() and np.isnan(got["mean"]).all() and (hist["majority"] == -1).all()
    # K = 0: nothing written, status OK
    z = eng.label_field_stats(np.full(N, -1, np.int32), field, K=0)
    assert all(z[k].shape == (0, 5) for k in STAT_KEYS) and z["n_skipped"] == 0
    z = eng.label_class_histogram(np.full(N, -1, np.int32), cls, 7, K=0)
    assert z["hist"].shape == (0, 7) and z["majority"].shape == (0,) and z["n_skipped"] == 0


# ---------------------------------------------------------------- 4. general floats
def _exact_square_parts(d):
    """d * d as an unevaluated sum p + e of two doubles (Veltkamp split, Dekker product): exact, so math.fsum over both gives sum d^2
    rounded once.  (The restatement of test_gpu_segment_fields.py's helper.)"""
    c = 134217729.0 * d
    hi = c - (c - d)
    lo = d - hi
    p = d * d
    e = ((hi * hi - p) + 2.0 * hi * lo) + lo * lo
    return p, e


def test_general_floats_within_the_summation_bound(gpu):
    """The three channels and the bound of test_gpu_segment_fields.py::test_general_floats_within_the_summation_bound, derived there from
    u = 2^-52 and n terms: |S1 - S1x| <= e1 = n u sum|d|, |S2 - S2x| <= e2 = n u sum d^2; the mean is off by at most e1 / n plus one
    rounding each of the quotient and the sum, the variance by e2 / n + 2 |m1| e1 / n plus one rounding of each of the quotient, the product
    and the difference; the reference's own last steps doubled in.  S1x and S2x are math.fsum over the exact differences and Dekker
    products -- not the code under test.  The labelling splits every segment of a town scene in three inside its voxels."""
    if "town" not in _cache:
        xyz = gpu.scenes.town_scene(60_000)
        _cache["town"] = (xyz, _engine(gpu, xyz))
    xyz, eng = _cache["town"]
    own = eng.point_labels()
    N = xyz.shape[0]
    labels = np.where(own >= 0, 3 * own + np.arange(N) % 3, -1).astype(np.int32)
    K = 3 * eng.counts()["kept"]
    rng = np.random.default_rng(14)
    field = np.stack([(1e9 + rng.normal(0, 1, N)).astype(np.float32), (1e4 + rng.normal(0, 1, N)).astype(np.float32),
                      rng.normal(0, 1, N).astype(np.float32)], axis=1)
    got = eng.label_field_stats(labels, field, K=K)
    lab_in, skipped = _inside(eng, labels)
    assert got["n_skipped"] == skipped
    order = np.argsort(lab_in, kind="stable")
    start = np.searchsorted(lab_in[order], np.arange(K + 1))
    worst, seen = 0.0, 0
    for k in range(K):
        idx = order[start[k]:start[k + 1]]
        n = idx.size
        assert n == got["n_valid"][k, 0]
        if n == 0:
            continue
        seen += 1
        for c in range(3):
            a = got["anchor"][k, c]
            dd = field[idx, c].astype(np.float64) - a
            p, e = _exact_square_parts(dd)
            s1x, s2x = math.fsum(dd), math.fsum(np.concatenate([p, e]))
            A1 = math.fsum(np.abs(dd))
            e1, e2 = n * U * A1, n * U * s2x
            m1x = s1x / n
            meanx, varx = a + m1x, max(0.0, s2x / n - m1x * m1x)
            tol_mean = e1 / n + 2 * U * (abs(m1x) + abs(meanx))
            tol_var = e2 / n + 2 * abs(m1x) * e1 / n + 4 * U * (s2x / n + m1x * m1x)
            em, ev = abs(got["mean"][k, c] - meanx), abs(got["var"][k, c] - varx)
            assert em <= tol_mean, (k, c, n, em, tol_mean)
            assert ev <= tol_var, (k, c, n, ev, tol_var)
            if tol_var > 0:
                worst = max(worst, ev / tol_var)
    print(f"largest var error / bound = {worst:.3g} over {seen} labels")
    assert seen > 10
    big = got["n_valid"][:, 1] >= 1000   # the shift does its work: a unit spread on an offset of 1e4 keeps its variance
    assert big.any() and (got["var"][big, 1] > 0.5).all() and (got["var"][big, 1] < 2.0).all()


# ---------------------------------------------------------------- 5. the anchor
def test_anchor_is_one_octree_point_of_the_label(gpu):
    xyz, labels, K, kw = _mixed_scenes()["tilted_planes"]
    eng = _engine(gpu, xyz, **kw)
    ch = 5
    field = _int_field(xyz.shape[0], ch, 9)
    rng = np.random.default_rng(10)
    field.reshape(-1)[rng.choice(field.size, field.size // 4, replace=False)] = np.nan   # many anchors meet an invalid value: 0.0 there
    got = eng.label_field_stats(labels, field, K=K)
    lab_in, _ = _inside(eng, labels)
    m = lab_in >= 0
    lab = lab_in[m].astype(np.int64)
    expect = np.where(np.isfinite(field[m]), field[m].astype(np.float64), 0.0)
    explains = (expect == got["anchor"][lab]).all(axis=1)           # this point explains every channel of its label's anchor row
    has = np.bincount(lab, minlength=K) > 0
    assert (np.bincount(lab[explains], minlength=K)[has] >= 1).all()
    assert (got["anchor"][has] == 0).any() and (got["anchor"] != 0).any()
    assert not has[K - 1] and (got["anchor"][~has] == 0).all()      # a label without a point: a zero anchor
    _check_exact(eng, labels, K, field)


# ---------------------------------------------------------------- 6. invalid values
def test_invalid_values_are_skipped(gpu):
    xyz, eng = _plain(gpu)
    N, ch, K = xyz.shape[0], 3, 6
    labels = (np.arange(N) % 7 - 1).astype(np.int32)       # labels -1 .. 5, alternating from point to point
    clean = _int_field(N, ch, 16)
    rng = np.random.default_rng(17)
    field = clean.copy()
    bad = rng.choice(N * ch, N * ch // 10, replace=False)
    field.reshape(-1)[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), bad.size)
    got, _, n_points = _check_exact(eng, labels, K, field)
    m = labels >= 0
    n_bad = np.stack([np.bincount(labels[m], weights=~np.isfinite(field[m, c]), minlength=K) for c in range(ch)], axis=1).astype(np.int64)
    assert n_bad.min() > 0 and np.array_equal(got["n_valid"], n_points[:, None] - n_bad)
    # an invalid value replaced by another invalid value: nothing changes, by bytes
    other = field.copy()
    flat = other.reshape(-1)
    flat[bad] = np.where(np.isnan(flat[bad]), np.float32(np.inf), np.float32(np.nan))
    assert not _diff(eng.label_field_stats(labels, other, K=K), got, STAT_KEYS)
    # one channel of one label invalid throughout: that entry is empty, every other entry stays, by bytes
    field2 = field.copy()
    field2[labels == 2, 1] = np.nan
    got2 = eng.label_field_stats(labels, field2, K=K)
    assert got2["n_valid"][2, 1] == 0 and got2["anchor"][2, 1] == 0 and all(np.isnan(got2[f][2, 1]) for f in ("mean", "var", "vmin", "vmax"))
    keep = np.ones((K, ch), dtype=bool)
    keep[2, 1] = False
    for f in STAT_KEYS:
        assert got2[f][keep].tobytes() == got[f][keep].tobytes(), f


# ---------------------------------------------------------------- 7. histogram specifics
@pytest.mark.parametrize("method", [2, 3], ids=["vgs", "svgs"])
def test_histogram_ties_outside_rows_and_point_counts(gpu, method):
    xyz, eng = _urban(gpu, method)
    N = xyz.shape[0]
    own = eng.point_labels()
    K = 3 * eng.counts()["kept"] + 1                                 # (the last label: no point)
    labels = np.where(own >= 0, 3 * own + np.arange(N) % 3, -1).astype(np.int32)
    if method == 3:
        labels[::2] = np.maximum(labels[::2], 0)                     # label points outside the supervoxels too: they are skipped
    n_classes = 9
    cls = _classes(N, n_classes, 60)
    lab_in, skipped = _inside(eng, labels)
    by_size = np.argsort(-np.bincount(lab_in[lab_in >= 0], minlength=K), kind="stable")
    k_out, k_tie = int(by_size[1]), int(by_size[2])
    cls[labels == k_out] = -1                                        # every class outside
    tie = np.nonzero(lab_in == k_tie)[0]
    assert tie.size >= 2
    cls[labels == k_tie] = n_classes                                 # (its points outside the octree: no part in the tie)
    cls[tie] = np.where(np.arange(tie.size) % 2 == 0, 5, 3)          # a tie of the two largest counts: the lower class wins
    if tie.size % 2:
        cls[tie[-1]] = n_classes
    _, hist, n_points = _check_exact(eng, labels, K, _int_field(N, 2, 61), cls, n_classes)
    print(f"method {method}: {skipped} labelled points outside the octree")
    assert skipped == 0 or method == 3
    assert hist["majority"][k_out] == -1 and hist["majority_count"][k_out] == 0 and hist["n_outside"][k_out] == n_points[k_out] > 0
    assert hist["hist"][k_tie, 3] == hist["hist"][k_tie, 5] == tie.size // 2 and hist["majority"][k_tie] == 3
    assert n_points[K - 1] == 0 and hist["majority"][K - 1] == -1


# ---------------------------------------------------------------- 8. labelled points outside the octree
def test_labelled_points_outside_the_octree_are_skipped(gpu):
    rng = np.random.default_rng(21)
    clean = gpu.scenes.town_scene(40_000)
    N = clean.shape[0]
    lab_clean = rng.integers(-1, 5, N).astype(np.int32)
    f_clean, c_clean = _int_field(N, 3, 22), _classes(N, 6, 23)
    at = np.sort(rng.choice(N, 60, replace=False))   # bad points in between, each with a label, field values and a class
    bad = np.full((60, 3), 1.0, np.float32)
    bad[0::3, 0], bad[1::3, 1], bad[2::3, 2] = np.nan, np.inf, -np.inf
    xyz = np.insert(clean, at, bad, axis=0)
    lab_bad = rng.integers(-1, 5, 60).astype(np.int32)
    labels = np.insert(lab_clean, at, lab_bad)
    field = np.insert(f_clean, at, _int_field(60, 3, 24), axis=0)
    cls = np.insert(c_clean, at, _classes(60, 6, 25))
    eng, eng_clean = _engine(gpu, xyz), _engine(gpu, clean)
    got, hist, _ = _check_exact(eng, labels, 5, field, cls, 6)
    assert got["n_skipped"] == hist["n_skipped"] == int((lab_bad >= 0).sum()) > 0
    # the rows of the clean points alone, by value ...
    ref = ref_field_stats(f_clean, lab_clean, 5, got["anchor"])
    assert all(np.array_equal(got[k], ref[k], equal_nan=True) for k in ("n_valid", "mean", "var", "vmin", "vmax"))
    rh = ref_class_hist(c_clean, lab_clean, 5, 6)
    assert all(np.array_equal(hist[k], rh[k]) for k in HIST_KEYS)
    # ... and by bytes the tables of an engine over the clean cloud: the same points in the same order, anchor included
    want, hwant = eng_clean.label_field_stats(lab_clean, f_clean, K=5), eng_clean.label_class_histogram(lab_clean, c_clean, 6, K=5)
    assert want["n_skipped"] == hwant["n_skipped"] == 0
    assert not _diff(got, want, STAT_KEYS) and not _diff(hist, hwant, HIST_KEYS)


# ---------------------------------------------------------------- 9. row permutation
def test_renaming_the_labels_permutes_the_rows(gpu):
    xyz, eng = _urban(gpu, 2)
    N = xyz.shape[0]
    own = eng.point_labels()
    K = 2 * eng.counts()["kept"]
    labels = np.where(own >= 0, 2 * own + np.arange(N) % 2, -1).astype(np.int32)
    pi = np.random.default_rng(8).permutation(K).astype(np.int32)
    renamed = np.where(labels >= 0, pi[np.maximum(labels, 0)], -1).astype(np.int32)
    field = np.random.default_rng(9).normal(3.0, 2.0, (N, 5)).astype(np.float32)
    cls = _classes(N, 7, 26)
    a, b = eng.label_field_stats(labels, field, K=K), eng.label_field_stats(renamed, field, K=K)
    for name in STAT_KEYS:
        assert b[name][pi].tobytes() == a[name].tobytes(), name
    a, b = eng.label_class_histogram(labels, cls, 7, K=K), eng.label_class_histogram(renamed, cls, 7, K=K)
    for name in HIST_KEYS:
        assert b[name][pi].tobytes() == a[name].tobytes(), name


# ---------------------------------------------------------------- 10. the refined labels
@pytest.mark.parametrize("name", ["dropped_beside_kept", "urban"])
def test_refined_labels_get_their_own_tables(gpu, name):
    if name == "urban":
        xyz, eng = _urban(gpu, 2)
    else:
        xyz = dropped_beside_kept()
        eng = _engine(gpu, xyz, **GROUP5)
    N, K = xyz.shape[0], eng.counts()["kept"]
    counts = eng.refine_labels()
    refined = eng.refined_labels()
    assert counts["points_filled"] > 0 and not np.array_equal(refined, eng.point_labels())
    before = helpers.snapshot(eng)
    field, cls = _int_field(N, 3, 27), _classes(N, 7, 28)
    got, hist, n_points = _check_exact(eng, refined, K, field, cls, 7)
    assert np.array_equal(n_points, np.bincount(refined[refined >= 0], minlength=K))
    # another labelling than the voxel labels': its tables are not theirs
    assert _diff(got, eng.segment_field_stats(field), STAT_KEYS) and _diff(hist, eng.segment_class_histogram(cls, 7), HIST_KEYS)
    assert np.array_equal(eng.refined_labels(), refined)
    helpers.assert_same_snapshot(helpers.snapshot(eng), before, "after label_field_stats / label_class_histogram")


# ---------------------------------------------------------------- 11. determinism and input forms
def test_two_calls_two_engines_and_every_input_form_give_the_same_bytes(gpu):
    torch = pytest.importorskip("torch")
    xyz, labels, K, kw = _mixed_scenes()["tilted_planes"]
    N, ch = xyz.shape[0], 5
    rng = np.random.default_rng(29)
    field = np.stack([1e9 + rng.normal(0, 1, N), rng.normal(0, 1, N), rng.uniform(0, 255, N), xyz[:, 2], rng.normal(5, 2, N)], axis=1).astype(np.float32)
    field[rng.choice(N, 100, replace=False), 1] = np.nan
    cls = _classes(N, 16, 31)
    a, b = _engine(gpu, xyz, **kw), _engine(gpu, xyz, **kw)
    first, hfirst = a.label_field_stats(labels, field, K=K), a.label_class_histogram(labels, cls, 16, K=K)
    assert not _diff(a.label_field_stats(labels, field, K=K), first, STAT_KEYS) and not _diff(b.label_field_stats(labels, field, K=K), first, STAT_KEYS)
    assert not _diff(a.label_class_histogram(labels, cls, 16, K=K), hfirst, HIST_KEYS)
    assert not _diff(b.label_class_histogram(labels, cls, 16, K=K), hfirst, HIST_KEYS)
    # a padded host stride, device tensors read in place, a padded device stride
    wide = np.full((N, ch + 3), np.float32(np.nan))
    wide[:, :ch] = field
    assert wide[:, :ch].strides == (4 * (ch + 3), 4)
    assert not _diff(a.label_field_stats(labels, wide[:, :ch], K=K), first, STAT_KEYS)
    dl, df, dc = (torch.from_numpy(x).to("cuda:0") for x in (labels, field, cls))
    assert not _diff(a.label_field_stats(dl, df, K=K), first, STAT_KEYS)
    dwide = torch.from_numpy(wide).to("cuda:0")[:, :ch]
    assert dwide.stride(0) == ch + 3 and not _diff(a.label_field_stats(dl, dwide, K=K), first, STAT_KEYS)
    assert not _diff(a.label_class_histogram(dl, dc, 16, K=K), hfirst, HIST_KEYS)
    assert not _diff(a.label_field_stats(labels, field[:, 2], K=K), a.label_field_stats(dl, df[:, 2].contiguous(), K=K), STAT_KEYS)


# ---------------------------------------------------------------- 12. the status contract
def _raw_stats(eng, labels, K, field, n, ch, stride):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return eng._L.vgs_point_label_field_stats(eng._h, p(labels), K, p(field), n, ch, stride, *([None] * 7))


def _raw_hist(eng, labels, K, cls, n, nc):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return eng._L.vgs_point_label_class_histogram(eng._h, p(labels), K, p(cls), n, nc, *([None] * 5))


def test_status_codes(gpu):
    torch = pytest.importorskip("torch")
    lib = gpu._lib
    xyz, eng = _plain(gpu)
    N = xyz.shape[0]
    labels = (np.arange(N) % 3).astype(np.int32)
    field, cls = _int_field(N, 4, 32), _classes(N, 5, 33)
    calls = {"fields": lambda e, l, K, n=None: e.label_field_stats(l, field[:n], K=K),
             "classes": lambda e, l, K, n=None: e.label_class_histogram(l, cls[:n], 5, K=K)}
    right = {"fields": lambda: _check_exact(eng, labels, 3, field), "classes": lambda: _check_exact(eng, labels, 3, field, cls, 5)}

    def refused(status, call, *words):
        with pytest.raises(gpu.VgsError) as e:
            call()
        assert e.value.status == status and all(w in str(e.value) for w in words), (status, words, str(e.value))

    for name, call in calls.items():
        # a label equal to K: the message names the smallest offending index and its value
        bad = labels.copy()
        bad[[150_001, 70_003]] = 3
        bad[190_000] = 9
        refused(lib.VGS_E_ARG, lambda: call(eng, bad, 3), "[70003] = 3", "K = 3")
        right[name]()
        refused(lib.VGS_E_ARG, lambda: call(eng, labels[:-1], 3), "n = " + str(N - 1))          # a wrong n: the labels ...
        refused(lib.VGS_E_ARG, lambda: call(eng, labels, 3, N - 1), "n = " + str(N - 1))        # ... and the attribute
        refused(lib.VGS_E_ARG, lambda: call(eng, labels, -1), "K = -1")
        right[name]()
        fresh = gpu.Engine(gpu.default_params(2))   # before run()
        fresh.set_points(xyz[:1000])
        refused(lib.VGS_E_STATE, lambda: call(fresh, labels[:1000], 3, 1000))
        fresh.voxelize(); fresh.features(); fresh.adjacency()
        refused(lib.VGS_E_STATE, lambda: call(fresh, labels[:1000], 3, 1000))
    # a NULL input
    assert _raw_stats(eng, None, 3, field, N, 4, 16) == lib.VGS_E_ARG and b"labels" in eng._L.vgs_last_error_string(eng._h)
    assert _raw_stats(eng, labels, 3, None, N, 4, 16) == lib.VGS_E_ARG
    assert _raw_hist(eng, None, 3, cls, N, 5) == lib.VGS_E_ARG and _raw_hist(eng, labels, 3, None, N, 5) == lib.VGS_E_ARG
    # channels, stride, classes
    refused(lib.VGS_E_ARG, lambda: eng.label_field_stats(labels, np.zeros((N, 0), np.float32), K=3), "n_channels")
    refused(lib.VGS_E_ARG, lambda: eng.label_field_stats(labels, np.zeros((N, 65), np.float32), K=3), "n_channels")
    for stride in (12, 4 * 4 + 2, 0, -16):          # below 4 * C; not a multiple of 4
        assert _raw_stats(eng, labels, 3, field, N, 4, stride) == lib.VGS_E_ARG, stride
        assert b"stride_bytes" in eng._L.vgs_last_error_string(eng._h)
    refused(lib.VGS_E_ARG, lambda: eng.label_class_histogram(labels, cls, 0, K=3), "n_classes")
    refused(lib.VGS_E_ARG, lambda: eng.label_class_histogram(labels, cls, 1025, K=3), "n_classes")
    assert _raw_stats(eng, labels, 3, field, N, 4, 16) == lib.VGS_OK and _raw_hist(eng, labels, 3, cls, N, 5) == lib.VGS_OK   # every output NULL
    assert eng.label_field_stats(labels, np.zeros((N, 64), np.float32), K=3)["mean"].shape == (3, 64)
    assert eng.label_class_histogram(labels, cls, 1024, K=3)["hist"].shape == (3, 1024)
    # the tables' limit: all labels -1 and a large K, so nothing large is built before the check; the numbers are in the message
    none = np.full(N, -1, np.int32)
    Kbig = (1 << 27) // 1024 + 1
    assert _raw_hist(eng, none, Kbig, cls, N, 1024) == lib.VGS_E_UNSUPPORTED
    msg = eng._L.vgs_last_error_string(eng._h).decode()
    assert str(Kbig) in msg and str(Kbig * 1024) in msg and str(1 << 27) in msg, msg
    assert _raw_stats(eng, none, (1 << 27) // 4 + 1, field, N, 4, 16) == lib.VGS_E_UNSUPPORTED
    msg = eng._L.vgs_last_error_string(eng._h).decode()
    assert str((1 << 27) // 4 + 1) in msg and str((1 << 27) + 4) in msg, msg
    # mixed numpy / torch inputs
    dl, df, dc = (torch.from_numpy(x).to("cuda:0") for x in (labels, field, cls))
    for call in (lambda: eng.label_field_stats(dl, field, K=3), lambda: eng.label_field_stats(labels, df, K=3),
                 lambda: eng.label_class_histogram(dl, cls, 5, K=3), lambda: eng.label_class_histogram(labels, dc, 5, K=3)):
        with pytest.raises(ValueError):
            call()
    # the device entry points check the same arguments
    refused(lib.VGS_E_ARG, lambda: eng.label_field_stats(dl[:-1], df[:-1], K=3), "n = ")
    refused(lib.VGS_E_ARG, lambda: eng.label_class_histogram(dl, dc, 1025, K=3), "n_classes")
    bad_dev = dl.clone()
    bad_dev[4242] = 3
    refused(lib.VGS_E_ARG, lambda: eng.label_field_stats(bad_dev, df, K=3), "[4242] = 3")
    for check in right.values():   # after every failure a valid call gives the right table
        check()
    # a tile context is refused: the tiled driver has no call for these tables yet
    t = gpu.Engine(gpu.default_params(2))
    t.set_points(xyz[:5000])
    lo, hi = np.array([-1e9, -1e9], dtype=np.float64), np.array([1e9, 1e9], dtype=np.float64)
    t._ck(t._L.vgs_set_owned_region(t._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    t.run()
    for call in calls.values():
        refused(lib.VGS_E_STATE, lambda: call(t, labels[:5000], 3, 5000), "tile context", "tiled driver")


# ---------------------------------------------------------------- 13. the front end
def test_vgs_run_writes_the_refined_attribute_tables(gpu, tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    n_classes = 6
    xyz = gpu.scenes.town_scene(60_000)
    N = xyz.shape[0]
    rng = np.random.default_rng(31)
    inten = rng.uniform(0.0, 1.0, N).astype(np.float32)
    inten[rng.choice(N, 50, replace=False)] = np.nan
    cls = rng.integers(0, n_classes + 2, N).astype(np.uint8)      # two classes outside the histogram
    gpu.pcd.write_pcd(tmp_path / "in.pcd", xyz, mode="binary", extra={"intensity": inten, "cls": cls})
    lines = dict(VGS_LINES)
    lines.update({12: str(tmp_path) + "/", 15: "in.pcd", 18: str(tmp_path) + "/", 21: "out.pcd"})
    _write_task(tmp_path / "task.txt", 2, lines)
    task = str(tmp_path / "task.txt")
    pf, pc, f, c, rf, rc, of, oc = (str(tmp_path / n) for n in ("pf.csv", "pc.csv", "f.csv", "c.csv", "rf.csv", "rc.csv", "of.csv", "oc.csv"))
    common = ["--fields", "intensity,z", "--class-field", "cls", "--classes", str(n_classes)]
    subprocess.check_call([RUN, task, "--refine", "--segment-fields", pf, "--segment-classes", pc] + common, stdout=subprocess.DEVNULL)
    subprocess.check_call([RUN, task, "--refine", "--segment-fields", f, "--segment-classes", c, "--refined-segment-fields", rf,
                           "--refined-segment-classes", rc] + common, stdout=subprocess.DEVNULL)
    for a, b in ((f, pf), (c, pc)):   # the voxel-label files do not depend on the new flags
        assert open(a, "rb").read() == open(b, "rb").read()
    # --fields / --class-field / --classes serve a refined file alone
    subprocess.check_call([RUN, task, "--refine", "--refined-segment-fields", of, "--refined-segment-classes", oc] + common, stdout=subprocess.DEVNULL)
    assert open(of, "rb").read() == open(rf, "rb").read() and open(oc, "rb").read() == open(rc, "rb").read()
    eng = _engine(gpu, xyz)
    eng.refine_labels()
    refined = eng.refined_labels()
    st = eng.label_field_stats(refined, np.stack([inten, xyz[:, 2]], axis=1))
    K = st["mean"].shape[0]
    assert K == eng.counts()["kept"] > 0 and (st["n_valid"][:, 0] < st["n_valid"][:, 1]).any()
    with open(rf) as fh:
        header = fh.readline().strip().split(",")
    assert header == ["label"] + [f"{n}_{s}" for n in ("intensity", "z") for s in ("n_valid", "mean", "var", "min", "max")]
    assert header == open(f).readline().strip().split(",")
    rows = np.loadtxt(rf, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    assert rows.shape == (K, 11) and np.array_equal(rows[:, 0], np.arange(K))
    for ch in range(2):
        o = 1 + 5 * ch
        assert np.array_equal(rows[:, o].astype(np.int64), st["n_valid"][:, ch])
        # %.17g doubles and %.9g floats read back exactly
        assert np.array_equal(rows[:, o + 1], st["mean"][:, ch], equal_nan=True) and np.array_equal(rows[:, o + 2], st["var"][:, ch], equal_nan=True)
        assert np.array_equal(rows[:, o + 3].astype(np.float32), st["vmin"][:, ch], equal_nan=True)
        assert np.array_equal(rows[:, o + 4].astype(np.float32), st["vmax"][:, ch], equal_nan=True)
    assert not np.array_equal(rows[:, 1], np.loadtxt(f, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)[:, 1])   # not the voxel labels' table
    h = eng.label_class_histogram(refined, cls.astype(np.int32), n_classes)
    with open(rc) as fh:
        header = fh.readline().strip().split(",")
    assert header == ["label", "majority", "majority_count", "n_outside"] + [f"hist_{j}" for j in range(n_classes)]
    rows = np.loadtxt(rc, delimiter=",", skiprows=1, dtype=np.int64, ndmin=2)
    assert rows.shape == (K, 4 + n_classes) and np.array_equal(rows[:, 0], np.arange(K))
    assert np.array_equal(rows[:, 1], h["majority"]) and np.array_equal(rows[:, 2], h["majority_count"])
    assert np.array_equal(rows[:, 3], h["n_outside"]) and np.array_equal(rows[:, 4:], h["hist"])
    assert h["n_outside"].sum() > 0
