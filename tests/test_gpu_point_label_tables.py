"""Descriptors, oriented boxes and scores of a caller's per-POINT labelling (vgs_point_label_descriptors, vgs_point_label_boxes,
vgs_compare_point_labels; csrc/pointseg.hip): Engine.describe_labels, label_boxes and compare_labels(ref, labels=...).

The main acceptance test: handed the engine's own point labels, the new pass returns the cached tables of segment_descriptors(),
segment_boxes() and compare_labels() byte for byte.  Then what no node-sorted pass can describe -- labels that alternate inside voxels --
against the float64 references (helpers.ref_descriptors with check_descriptors' tolerances, segment_boxes_ref.ref_boxes to the bit,
label_compare_ref.compare_labels to the bit); segments at the chunk and fold limits (SD_CHUNK = 2048 points per chunk, 64 partials per
fold step: csrc/vgs_context.hpp), empty labels, K = 1 and 0; row permutation; the refined labels; skipped points; a scene far from the
origin; determinism and the status contract."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import label_compare_ref as R
from label_refine_scenes import GROUP5, big_boundary_voxel, dropped_beside_kept
from segment_boxes_ref import ref_boxes
from segment_scenes import FAR, SPLIT, two_tilted_planes
from test_cpp_segment_desc import CSRC, RUN, VGS_LINES, _write_task

pytestmark = pytest.mark.gpu

SD_CHUNK = 2048   # points per chunk (csrc/vgs_context.hpp: SD_TB * SD_PPT)
FRAMES = ("principal", "upright")
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


def _same_bytes(a, b, names):
    return [n for n in names if not (a[n].dtype == b[n].dtype and a[n].shape == b[n].shape and a[n].tobytes() == b[n].tobytes())]


DESC = [n for n, _, _ in (("n_points", 0, 0), ("n_nodes", 0, 0), ("bbox6", 0, 0), ("centroid3", 0, 0), ("cov6", 0, 0), ("evals3", 0, 0),
                          ("evecs9", 0, 0), ("eigen8", 0, 0))]
BOX = ["center3", "half3", "frame9", "lo3", "hi3"]


def _check_rows(eng, xyz, labels, K, svgs=False):
    """describe_labels and label_boxes of an arbitrary labelling against the float64 references: counts, node counts and boxes exact, the
    fp64 fields within helpers.check_descriptors' tolerances, the extents to the bit; a label no point carries by the header's rule."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    got = eng.describe_labels(labels, K=K)
    pv = eng.point_voxel()
    inside = pv >= 0
    lab_in = np.where(inside, labels, -1).astype(np.int32)
    assert got["n_skipped"] == int(((labels >= 0) & ~inside).sum())
    ref = helpers.ref_descriptors(xyz, lab_in, K)
    n = ref["n_points"]
    assert np.array_equal(got["n_points"], n) and got["n_points"].dtype == np.int64
    m = lab_in >= 0
    pairs = np.unique(np.stack([lab_in[m].astype(np.int64), pv[m].astype(np.int64)], axis=1), axis=0)
    assert np.array_equal(got["n_nodes"], np.bincount(pairs[:, 0], minlength=K).astype(np.int32))
    assert helpers.same_box(got["bbox6"], ref["bbox6"], ref["zero_signs"])
    has = n > 0
    c = got["centroid3"]
    assert (np.abs(c - ref["centroid3"])[has] <= (1e-9 * (1 + np.linalg.norm(ref["centroid3"], axis=1))[:, None])[has]).all()
    tr = ref["cov6"][:, [0, 3, 5]].sum(axis=1)
    assert (np.abs(got["cov6"] - ref["cov6"])[has] <= (1e-8 * tr[:, None] + 1e-30)[has]).all()
    lmax = ref["evals3"][:, 2]
    assert (got["evals3"] >= 0).all() and (np.diff(got["evals3"], axis=1) >= 0).all()
    assert (np.abs(got["evals3"] - np.maximum(ref["evals3"], 0))[has] <= (1e-8 * lmax[:, None] + 1e-30)[has]).all()
    V = got["evecs9"].reshape(K, 3, 3)
    assert np.allclose(np.einsum("kri,krj->kij", V, V), np.eye(3)[None], atol=1e-10)
    for j in range(3):
        col = V[:, :, j]
        assert (col[np.arange(K), np.argmax(np.abs(col), axis=1)] > 0).all(), j
        w = ref["evals3"]
        with np.errstate(invalid="ignore"):
            gap = np.minimum(np.abs(w[:, j] - w[:, j - 1]) if j > 0 else np.inf, np.abs(w[:, j + 1] - w[:, j]) if j < 2 else np.inf)
            sel = has & (gap >= 1e-3 * lmax)
        dots = np.abs((col * ref["evecs"][:, :, j]).sum(axis=1))
        assert (dots[sel] >= 1 - 1e-6).all(), (j, dots[sel].min())
    few = n <= 1
    assert (got["cov6"][few] == 0).all() and (got["eigen8"][few] == 0).all() and (V[few] == np.eye(3)[None]).all()
    np.testing.assert_allclose(got["eigen8"], helpers.ref_features(got["evals3"], svgs), rtol=1e-5, atol=1e-6)
    # a label no point carries
    e = ~has
    assert (got["n_nodes"][e] == 0).all() and (got["centroid3"][e] == 0).all() and (got["evals3"][e] == 0).all()
    assert (got["bbox6"][e, :3] == np.inf).all() and (got["bbox6"][e, 3:] == -np.inf).all()
    # boxes: the frames come from the rows above; the extents are an exact function of the points, the centroid and the frame
    occ = np.flatnonzero(has)
    remap = np.full(K + 1, -1, np.int32)
    remap[occ] = np.arange(occ.size, dtype=np.int32)
    for frame in FRAMES:
        b = eng.label_boxes(labels, frame, K=K)
        if frame == "principal":
            assert b["frame9"].tobytes() == got["evecs9"].tobytes()
        else:
            assert (b["frame9"][:, [2, 5, 6, 7]] == 0).all() and (b["frame9"][:, 8] == 1).all()
        if occ.size:
            rb = ref_boxes(xyz, remap[lab_in], occ.size, got["centroid3"][occ], b["frame9"][occ])
            for name in ("lo3", "hi3", "half3", "center3"):
                assert (b[name][occ] == rb[name]).all(), (frame, name)
        for name in ("lo3", "hi3", "half3"):
            assert (b[name][e] == 0).all(), (frame, name)
        assert (b["center3"][e] == got["centroid3"][e]).all()
    return got


# ---------------------------------------------------------------- 1. byte equality with the cached tables
@pytest.mark.parametrize("method", [2, 3], ids=["vgs", "svgs"])
def test_own_point_labels_reproduce_the_cached_tables(gpu, method):
    torch = pytest.importorskip("torch")
    xyz, eng = _urban(gpu, method)
    labels, K = eng.point_labels(), eng.counts()["kept"]
    assert K > 10
    dev = torch.from_numpy(labels).to("cuda:0")
    want = eng.segment_descriptors()
    for src in (labels, dev):
        got = eng.describe_labels(src)
        assert got["n_skipped"] == 0
        assert not _same_bytes({k: v.view(np.uint8) for k, v in got.items() if k in DESC}, {k: v.view(np.uint8) for k, v in want.items()}, DESC)
        for frame in FRAMES:
            assert not _same_bytes(eng.label_boxes(src, frame), eng.segment_boxes(frame), BOX), frame
    ref = (np.arange(labels.size) % 211 - 3).astype(np.int32)
    plain = eng.compare_labels(ref)
    assert R.same(eng.compare_labels(ref, labels=labels), plain)
    assert R.same(eng.compare_labels(torch.from_numpy(ref).to("cuda:0"), labels=dev), plain)
    assert R.same(eng.compare_labels(ref), plain)


# ---------------------------------------------------------------- 2. and 7. labels that alternate inside voxels, near and far
def _mixed_scenes():
    a = big_boundary_voxel()
    la = (np.arange(a.shape[0]) % 3).astype(np.int32)
    b = two_tilted_planes()
    side = (b[:, 0] + 0.37 * b[:, 1] > 2.9).astype(np.int32)   # a plane that cuts through voxels
    lb = (np.arange(b.shape[0]) % 3 + 3 * side).astype(np.int32)
    return {"boundary_voxel": (a, la, 3, SPLIT), "tilted_planes": (b, lb, 7, {})}   # (label 6 of the planes: no point)


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
    got = _check_rows(eng, xyz, labels, K)
    assert (got["n_points"][:3] > 0).all()


# ---------------------------------------------------------------- 3. chunk and fold limits
def _plain(gpu):
    if "plain" not in _cache:
        xyz = np.random.default_rng(77).uniform(0.0, 6.0, size=(200_000, 3)).astype(np.float32)
        _cache["plain"] = (xyz, _engine(gpu, xyz))
    return _cache["plain"]


def test_chunk_and_fold_limits(gpu):
    xyz, eng = _plain(gpu)
    N = xyz.shape[0]
    sizes = {0: 1, 2: SD_CHUNK - 1, 3: SD_CHUNK, 6: SD_CHUNK + 1, 7: 140_000}   # 140 000 > 64 * SD_CHUNK: the lane-stride fold wraps
    K = 9                                                                         # labels 1, 4, 5 and the last one, 8: no point
    assert sizes[7] > 64 * SD_CHUNK
    labels = np.full(N, -1, np.int32)
    at = 11
    for k, n in sizes.items():
        labels[at:at + n] = k
        at += n + 5
    got = _check_rows(eng, xyz, labels, K)
    assert got["n_points"].tolist() == [1, 0, SD_CHUNK - 1, SD_CHUNK, 0, 0, SD_CHUNK + 1, 140_000, 0]
    # K = 1: everything one segment; and one segment of one chunk
    _check_rows(eng, xyz, np.zeros(N, np.int32), 1)
    one = np.full(N, -1, np.int32)
    one[5:900] = 0
    _check_rows(eng, xyz, one, 1)
    # every label -1: all rows empty
    none = _check_rows(eng, xyz, np.full(N, -7, np.int32), 4)
    assert not none["n_points"].any()
    # K = 0: nothing written, status OK
    z = eng.describe_labels(np.full(N, -1, np.int32), K=0)
    assert z["n_points"].shape == (0,) and z["bbox6"].shape == (0, 6) and z["n_skipped"] == 0
    assert eng.label_boxes(np.full(N, -1, np.int32), K=0)["lo3"].shape == (0, 3)
    c = eng.compare_labels(np.zeros(N, np.int32), labels=np.full(N, -1, np.int32), K=0)
    assert R.same(c, R.compare_labels(np.full(N, -1, np.int32), np.zeros(N, np.int32), 0))


# ---------------------------------------------------------------- 4. row permutation
def test_renaming_the_labels_permutes_the_rows(gpu):
    xyz, eng = _urban(gpu, 2)
    labels, K = eng.point_labels(), eng.counts()["kept"]
    pi = np.random.default_rng(8).permutation(K).astype(np.int32)
    renamed = np.where(labels >= 0, pi[np.maximum(labels, 0)], -1).astype(np.int32)
    a, b = eng.describe_labels(labels), eng.describe_labels(renamed)
    for name in DESC:
        assert b[name][pi].tobytes() == a[name].tobytes(), name
    for frame in FRAMES:
        a, b = eng.label_boxes(labels, frame), eng.label_boxes(renamed, frame)
        for name in BOX:
            assert b[name][pi].tobytes() == a[name].tobytes(), (frame, name)


# ---------------------------------------------------------------- 5. the refined labels
@pytest.mark.parametrize("name", ["dropped_beside_kept", "urban"])
def test_refined_labels_are_described_and_scored(gpu, name):
    if name == "urban":
        xyz, eng = _urban(gpu, 2)
    else:
        xyz = dropped_beside_kept()
        eng = _engine(gpu, xyz, **GROUP5)
    K = eng.counts()["kept"]
    counts = eng.refine_labels()
    refined = eng.refined_labels()
    assert counts["points_filled"] > 0 and not np.array_equal(refined, eng.point_labels())
    before = helpers.snapshot(eng)
    cached = eng.segment_descriptors()
    got = _check_rows(eng, xyz, refined, K)
    assert np.array_equal(got["n_points"], np.bincount(refined[refined >= 0], minlength=K))
    assert _same_bytes(got, cached, DESC)   # (the refined result is another labelling: its table is not the cached one)
    truth = (np.arange(xyz.shape[0]) // 97 % 23 - 1).astype(np.int32)
    assert R.same(eng.compare_labels(truth, labels=refined), R.compare_labels(refined, truth, K))
    assert np.array_equal(eng.refined_labels(), refined)
    assert not _same_bytes(eng.segment_descriptors(), cached, DESC)
    helpers.assert_same_snapshot(helpers.snapshot(eng), before, "after describe_labels / label_boxes / compare_labels(labels=)")


# ---------------------------------------------------------------- 6. skipped points
def test_labelled_points_outside_the_octree_are_skipped(gpu):
    rng = np.random.default_rng(21)
    clean = gpu.scenes.town_scene(40_000)
    N = clean.shape[0]
    lab_clean = rng.integers(-1, 5, N).astype(np.int32)
    at = np.sort(rng.choice(N, 60, replace=False))   # bad points in between, each with a label
    bad = np.full((60, 3), 1.0, np.float32)
    bad[0::3, 0], bad[1::3, 1], bad[2::3, 2] = np.nan, np.inf, -np.inf
    xyz = np.insert(clean, at, bad, axis=0)
    lab_bad = rng.integers(-1, 5, 60).astype(np.int32)
    labels = np.insert(lab_clean, at, lab_bad)
    eng, eng_clean = _engine(gpu, xyz), _engine(gpu, clean)
    got, want = eng.describe_labels(labels, K=5), eng_clean.describe_labels(lab_clean, K=5)
    assert got["n_skipped"] == int((lab_bad >= 0).sum()) > 0 and want["n_skipped"] == 0
    # the same points in the same order: equal rows (the node ids may differ between the two engines, their number per label does not)
    assert not _same_bytes(got, want, DESC)
    for frame in FRAMES:
        assert not _same_bytes(eng.label_boxes(labels, frame, K=5), eng_clean.label_boxes(lab_clean, frame, K=5), BOX)
    _check_rows(eng, xyz, labels, 5)
    # the comparison is index-wise: the bad points take part with the label the caller gave them
    truth = rng.integers(-1, 9, labels.size).astype(np.int32)
    assert R.same(eng.compare_labels(truth, labels=labels, K=5), R.compare_labels(labels, truth, 5))


# ---------------------------------------------------------------- 8. determinism and contract
def test_two_calls_and_two_engines_give_the_same_bytes(gpu):
    xyz, labels, K, kw = _mixed_scenes()["tilted_planes"]
    a, b = _engine(gpu, xyz, **kw), _engine(gpu, xyz, **kw)
    first = a.describe_labels(labels, K=K)
    assert not _same_bytes(a.describe_labels(labels, K=K), first, DESC) and not _same_bytes(b.describe_labels(labels, K=K), first, DESC)
    for frame in FRAMES:
        f = a.label_boxes(labels, frame, K=K)
        assert not _same_bytes(a.label_boxes(labels, frame, K=K), f, BOX) and not _same_bytes(b.label_boxes(labels, frame, K=K), f, BOX)


def test_status_codes(gpu):
    lib = gpu._lib
    xyz, eng = _plain(gpu)
    N = xyz.shape[0]
    labels = np.zeros(N, np.int32)
    ref = np.zeros(N, np.int32)
    calls = {"describe": lambda e, l, **kw: e.describe_labels(l, **kw), "boxes": lambda e, l, **kw: e.label_boxes(l, **kw),
             "compare": lambda e, l, **kw: e.compare_labels(ref[:l.shape[0]], labels=l, **kw)}
    for name, call in calls.items():
        # a label equal to K: the message names the first offending index and its value
        bad = labels.copy()
        bad[[150_001, 70_003]] = 3
        bad[190_000] = 9
        with pytest.raises(gpu.VgsError) as e:
            call(eng, bad, K=3)
        assert e.value.status == lib.VGS_E_ARG and "[70003] = 3" in str(e.value) and "K = 3" in str(e.value), (name, str(e.value))
        with pytest.raises(gpu.VgsError) as e:   # wrong n
            call(eng, labels[:-1], K=3)
        assert e.value.status == lib.VGS_E_ARG, name
        with pytest.raises(gpu.VgsError) as e:   # negative K
            call(eng, labels, K=-1)
        assert e.value.status == lib.VGS_E_ARG, name
        fresh = gpu.Engine(gpu.default_params(2))   # before run()
        fresh.set_points(xyz[:1000])
        with pytest.raises(gpu.VgsError) as e:
            call(fresh, labels[:1000], K=3)
        assert e.value.status == lib.VGS_E_STATE, name
        fresh.voxelize(); fresh.features(); fresh.adjacency()
        with pytest.raises(gpu.VgsError) as e:
            call(fresh, labels[:1000], K=3)
        assert e.value.status == lib.VGS_E_STATE, name
    for frame in (2, -1):
        with pytest.raises(gpu.VgsError) as e:
            eng.label_boxes(labels, frame, K=3)
        assert e.value.status == lib.VGS_E_ARG
    # the refused calls left the context usable and its last comparison alone
    plain = eng.compare_labels(ref)
    with pytest.raises(gpu.VgsError):
        eng.compare_labels(ref, labels=np.full(N, 5, np.int32), K=3)
    out = {name: np.zeros(plain[name].shape, plain[name].dtype) for name, _, _ in gpu.Engine.COMPARE_FIELDS}
    eng._ck(eng._L.vgs_get_label_comparison(eng._h, *(out[name].ctypes.data_as(C.c_void_p) for name, _, _ in gpu.Engine.COMPARE_FIELDS)))
    assert all(out[name].tobytes() == plain[name].tobytes() for name in out)
    # a tile context is refused
    t = gpu.Engine(gpu.default_params(2))
    t.set_points(xyz[:5000])
    lo, hi = np.array([-1e9, -1e9], dtype=np.float64), np.array([1e9, 1e9], dtype=np.float64)
    t._ck(t._L.vgs_set_owned_region(t._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    t.run()
    for name, call in calls.items():
        with pytest.raises(gpu.VgsError) as e:
            call(t, labels[:5000], K=3)
        assert e.value.status == lib.VGS_E_STATE and "tile context" in str(e.value), name


# ---------------------------------------------------------------- the front end: vgs_run --refine --segments a.csv --refined-segments b.csv
def test_vgs_run_writes_both_tables(gpu, tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    xyz = gpu.scenes.town_scene(60_000)
    gpu.pcd.write_pcd(tmp_path / "in.pcd", xyz, mode="binary")
    lines = dict(VGS_LINES)
    lines.update({12: str(tmp_path) + "/", 15: "in.pcd", 18: str(tmp_path) + "/", 21: "out.pcd"})
    _write_task(tmp_path / "task.txt", 2, lines)
    plain, a, b = tmp_path / "plain.csv", tmp_path / "a.csv", tmp_path / "b.csv"
    subprocess.check_call([RUN, str(tmp_path / "task.txt"), "--refine", "--segments", str(plain)], stdout=subprocess.DEVNULL)
    subprocess.check_call([RUN, str(tmp_path / "task.txt"), "--refine", "--segments", str(a), "--refined-segments", str(b)], stdout=subprocess.DEVNULL)
    assert a.read_bytes() == plain.read_bytes()   # the --segments file does not depend on the new flag
    eng = _engine(gpu, xyz)
    eng.refine_labels()
    d = eng.describe_labels(eng.refined_labels())
    rows = np.loadtxt(b, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    K = d["n_points"].shape[0]
    assert rows.shape == (K, 29) and np.array_equal(rows[:, 0], np.arange(K))
    assert np.array_equal(rows[:, 1].astype(np.int64), d["n_points"]) and np.array_equal(rows[:, 2].astype(np.int32), d["n_nodes"])
    assert np.array_equal(rows[:, 3:9].astype(np.float32), d["bbox6"])
    assert np.array_equal(rows[:, 9:12], d["centroid3"]) and np.array_equal(rows[:, 12:15], d["evals3"])
    V = d["evecs9"].reshape(K, 3, 3)
    assert np.array_equal(rows[:, 15:18], V[:, :, 0]) and np.array_equal(rows[:, 18:21], V[:, :, 2])
    assert np.array_equal(rows[:, 21:29].astype(np.float32), d["eigen8"])
    assert not np.array_equal(rows[:, 1], np.loadtxt(a, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)[:, 1])
    assert os.path.exists(tmp_path / "out.pcd")
