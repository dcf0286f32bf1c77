"""The label comparison on the device (vgs_compare_labels, vgs_get_label_comparison; csrc/segcompare.hip): the sparse contingency table
between the engine's point labels and a reference labelling, the reference table, the segment table and the summary -- every array equal
to the numpy restatement tests/label_compare_ref.py, dtype and bytes (integers and single fp64 quotients: no tolerance anywhere).
Reference labellings are built from the engine's own labels and the point index, so that single segments hold exactly 0, 1, 63, 64, 65
and 257 distinct ids (the lane-stride loops of the row kernels: no cell, one, one short of a wavefront, a wavefront, one more, several
chunks), plus: every point its own id, one id, ids 0 and INT32_MAX, negative ids mixed in, all negative, engineered ties.
Then the identities (class histogram, ref = labels), the device variant, determinism, no side effects, the state and argument contract,
a reused context, and the C++ mirror through vgs_run's CSVs."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import label_compare_ref as R
from segment_scenes import GROUP, SPLIT, big_nodes, degenerate_scene, fragmented_plane

pytestmark = pytest.mark.gpu

INT32_MAX = np.iinfo(np.int32).max
INT32_MIN = np.iinfo(np.int32).min
TARGETS = (257, 65, 64, 63, 1, 0)   # distinct ids of the six largest segments of the "structured" labelling

SCENES = {
    "big_nodes": lambda gpu: (big_nodes(), 2, GROUP),
    "degenerate": lambda gpu: (degenerate_scene()[0], 2, GROUP),
    "fragmented": lambda gpu: (fragmented_plane(side=48), 2, SPLIT),
    "town": lambda gpu: (gpu.scenes.town_scene(60_000), 2, {}),
    "pc_svgs": lambda gpu: (gpu.scenes.pc_scene(60_000), 3, {}),
}
LARGE = ("big_nodes", "town", "pc_svgs")   # scenes with six segments of at least 257 points
_cache = {}


def _engine(gpu, xyz, method=2, **kw):
    eng = gpu.Engine(gpu.default_params(method, **kw))
    eng.set_points(xyz)
    eng.run()
    return eng


def _rank_in_segment(labels):
    """per point: its rank among the points of its label, in index order (the -1 points among themselves)"""
    order = np.argsort(labels, kind="stable")
    sl = labels[order]
    first = np.searchsorted(sl, sl, side="left")
    rank = np.empty(labels.size, np.int64)
    rank[order] = np.arange(labels.size) - first
    return rank


def _labellings(labels, K):
    """name -> int32 reference ids, from the labels and the point index alone"""
    N = labels.size
    idx = np.arange(N, dtype=np.int64)
    rank = _rank_in_segment(labels)
    size = np.bincount(labels[labels >= 0], minlength=max(K, 1))[:K] if K else np.zeros(0, np.int64)
    by_size = np.argsort(-size, kind="stable")
    out = {}
    # the six largest segments get min(target, size) distinct ids of their own; pairs of the others share an id, and so do the dropped points
    s = np.where(labels >= 0, 5000 + (labels.astype(np.int64) // 2) * 3, idx % 5)
    for j, m in enumerate(TARGETS[:min(K, len(TARGETS))]):
        sel = labels == by_size[j]
        s[sel] = (100_000 * (j + 1) + rank[sel] % m) if m else -1
    out["structured"] = s
    out["own_id"] = idx
    out["one_id"] = np.full(N, 5, np.int64)
    out["zero_and_max"] = np.where(idx % 2 == 0, 0, INT32_MAX)
    rng = np.random.default_rng(40)
    m = rng.integers(-3, 50, N)
    m[rng.choice(N, max(N // 20, 1), replace=False)] = INT32_MIN
    out["mixed_negative"] = m
    a = np.full(N, -1, np.int64)
    a[::3] = INT32_MIN
    out["all_negative"] = a
    # ties: in segment A (the largest) c points of id 7 and c of id 3, in segment B (the second) c points of id 7 and the rest without
    # annotation; everything else an id per segment.  Id 3 wins A (the lowest id), the lower of A and B wins id 7 (the lowest label).
    t = np.where(labels >= 0, 100 + labels.astype(np.int64), 50)
    if K >= 2:
        A, B = int(by_size[0]), int(by_size[1])
        c = int(min(size[A], size[B]) // 2)
        ra, rb = rank[labels == A], rank[labels == B]
        t[labels == A] = np.where(ra < c, 7, np.where(ra < 2 * c, 3, -1))
        t[labels == B] = np.where(rb < c, 7, -1)
    out["ties"] = t
    out["labels"] = labels.astype(np.int64)
    return {k: np.ascontiguousarray(v.astype(np.int32)) for k, v in out.items()}


def _scene(gpu, name):
    """(points, segmented engine, point labels, K, labellings) of a scene, made once and shared; the tests leave it segmented and unchanged"""
    if name not in _cache:
        xyz, method, kw = SCENES[name](gpu)
        eng = _engine(gpu, xyz, method, **kw)
        labels, K = eng.point_labels(), eng.counts()["kept"]
        _cache[name] = (xyz, eng, labels, K, _labellings(labels, K))
    return _cache[name]


def _restated(name, which):
    """the numpy restatement of a (scene, labelling) pair, computed once"""
    key = (name, which, "ref")
    if key not in _cache:
        _, _, labels, K, refs = _cache[name]
        _cache[key] = R.compare_labels(labels, refs[which], K)
    return _cache[key]


LABELLINGS = ("structured", "own_id", "one_id", "zero_and_max", "mixed_negative", "all_negative", "ties", "labels")


# ---------------------------------------------------------------- 1. the scenes reach the row lengths they are here for
@pytest.mark.parametrize("name", LARGE)
def test_single_segments_reach_the_distinct_id_counts(gpu, name):
    _, eng, labels, K, refs = _scene(gpu, name)
    size = np.bincount(labels[labels >= 0], minlength=K)
    assert K >= len(TARGETS) and np.sort(size)[-len(TARGETS)] >= 257
    by_size = np.argsort(-size, kind="stable")[:len(TARGETS)]
    want = _restated(name, "structured")
    assert want["seg_refs"][by_size].tolist() == list(TARGETS)
    got = eng.compare_labels(refs["structured"])
    assert got["seg_refs"][by_size].tolist() == list(TARGETS)
    assert got["seg_best_ref"][by_size[-1]] == -1 and got["seg_annotated"][by_size[-1]] == 0
    if name == "town":
        assert (labels == -1).any() and got["summary"][2] > 0 and (got["cell_seg"] == -1).sum() == 5


# ---------------------------------------------------------------- 2. every array equals the restatement
@pytest.mark.parametrize("which", LABELLINGS)
@pytest.mark.parametrize("name", list(SCENES))
def test_tables_equal_the_restatement(gpu, name, which):
    xyz, eng, labels, K, refs = _scene(gpu, name)
    ref = refs[which]
    got, want = eng.compare_labels(ref), _restated(name, which)
    assert R.same(got, want), (R.diff(got, want), got["summary"], want["summary"])
    s, N = got["summary"], labels.size
    assert got["seg_annotated"].shape == (K,) and s[0] + s[1] == N and s[11] == 0
    if which == "own_id":
        assert s[4] == N == s[3] and (got["cell_n"] == 1).all() and s[8] == 0
    if which == "one_id":
        assert s[3] == 1 and got["ref_id"].tolist() == [5] and got["ref_points"].tolist() == [N]
    if which == "zero_and_max":
        assert got["ref_id"].tolist() == [0, INT32_MAX] and got["cell_ref"].max() == INT32_MAX
    if which == "mixed_negative":
        assert s[1] > N // 20 and got["ref_id"].min() == 0
    if which == "all_negative":
        assert s.tolist() == [0, N] + [0] * 10 and got["cell_n"].size == 0 and got["ref_id"].size == 0
        assert (got["seg_best_ref"] == -1).all() and not got["seg_best_iou"].any() and not got["seg_refs"].any()
    if which == "ties" and K >= 2:
        size = np.bincount(labels[labels >= 0], minlength=K)
        A, B = (int(v) for v in np.argsort(-size, kind="stable")[:2])
        c = int(min(size[A], size[B]) // 2)
        if c > 0:
            assert got["seg_best_ref"][A] == 3 and got["seg_best_n"][A] == c and got["seg_refs"][A] == 2   # ids 3 and 7 tie: the lowest id
            row = int(np.searchsorted(got["ref_id"], 7))
            assert got["ref_id"][row] == 7 and got["ref_points"][row] == 2 * c
            assert got["ref_best_seg"][row] == min(A, B) and got["ref_best_n"][row] == c                  # A and B tie: the lowest label


# ---------------------------------------------------------------- 3. identities
@pytest.mark.parametrize("name", list(SCENES))
def test_cells_are_the_nonzero_entries_of_the_class_histogram(gpu, name):
    _, eng, labels, K, _ = _scene(gpu, name)
    N = labels.size
    ids = ((np.arange(N, dtype=np.int64) * 2654435761) % 1031 - 7).astype(np.int32)     # -7 .. 1023
    ids[ids >= 1024] = -1
    got = eng.compare_labels(ids)
    h = eng.segment_class_histogram(ids, 1024)
    kk, jj = np.nonzero(h["hist"])                      # row-major: ascending (segment, class), the order of the cells
    kept = got["cell_seg"] >= 0
    assert np.array_equal(got["cell_seg"][kept], kk) and np.array_equal(got["cell_ref"][kept], jj)
    assert np.array_equal(got["cell_n"][kept], h["hist"][kk, jj])
    assert np.array_equal(got["seg_best_ref"], h["majority"]) and np.array_equal(got["seg_best_n"], h["majority_count"])
    assert np.array_equal(got["seg_annotated"] + h["n_outside"], np.bincount(labels[labels >= 0], minlength=K))


@pytest.mark.parametrize("name", list(SCENES))
def test_reference_equal_to_the_labels_is_a_perfect_match(gpu, name):
    _, eng, labels, K, refs = _scene(gpu, name)
    got = eng.compare_labels(refs["labels"])            # dropped points carry -1: not annotated
    assert K > 0 and (got["seg_best_iou"] == 1.0).all() and (got["ref_best_iou"] == 1.0).all()
    assert np.array_equal(got["seg_best_ref"], np.arange(K)) and np.array_equal(got["ref_best_seg"], np.arange(K))
    assert got["summary"][2] == 0 and got["summary"][1] == int((labels < 0).sum())
    s = gpu.comparison_scores(got)
    assert s["matched"] == K and s["precision"] == 1.0 and s["recall"] == 1.0 and s["f1"] == 1.0
    assert s["purity"] == 1.0 and s["completeness"] == 1.0 and s["ari"] == 1.0


# ---------------------------------------------------------------- 4. device variant, determinism, isolation
@pytest.mark.parametrize("name", list(SCENES))
def test_device_tensor_and_second_call_give_the_same_bytes(gpu, name):
    torch = pytest.importorskip("torch")
    _, eng, labels, K, refs = _scene(gpu, name)
    for which in ("structured", "mixed_negative", "own_id"):
        host = eng.compare_labels(refs[which])
        assert R.same(host, eng.compare_labels(torch.from_numpy(refs[which]).to("cuda:0"))), which
        assert R.same(host, eng.compare_labels(refs[which])), which
    ptrs = eng.label_comparison_device()
    assert sorted(ptrs) == sorted(n for n, _, _ in gpu.Engine.COMPARE_FIELDS) and all(p for p in ptrs.values())
    eng.compare_labels(refs["all_negative"])
    ptrs = eng.label_comparison_device()
    assert ptrs["cell_n"] is None and ptrs["ref_id"] is None and ptrs["seg_annotated"]


def _others(eng):
    off, idx = eng.clusters()
    d, g = eng.segment_descriptors(), eng.segment_graph()
    b = {f: eng.segment_boxes(f) for f in ("principal", "upright")}
    return ([off, idx, eng.point_labels()] + [d[k] for k in sorted(d)] + [g[k] for k in sorted(g)] +
            [b[f][k] for f in sorted(b) for k in sorted(b[f])])


def _eq(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_second_engine_same_bytes_and_no_side_effects(gpu):
    xyz, e1, labels, K, refs = _scene(gpu, "town")
    before = _others(e1)
    c1 = {w: e1.compare_labels(refs[w]) for w in ("structured", "ties", "own_id")}
    assert _eq(before, _others(e1))                     # labels and cached tables: byte for byte what they were
    e2 = _engine(gpu, xyz)                              # engine to engine; here the compare comes before any other getter
    for w, c in c1.items():
        assert R.same(c, e2.compare_labels(refs[w])), w
    assert _eq(before, _others(e2))
    assert R.same(c1["own_id"], e2.compare_labels(refs["own_id"]))   # ... and after them


# ---------------------------------------------------------------- 5. state and argument contract
def _raw_get(eng):
    return eng._L.vgs_get_label_comparison(eng._h, *([None] * 14))


def test_state_and_argument_contract(gpu):
    lib = gpu._lib
    xyz = gpu.scenes.town_scene(60_000)
    N = xyz.shape[0]
    ref = (np.arange(N) % 11).astype(np.int32)
    eng = gpu.Engine(gpu.default_params(2))
    with pytest.raises(gpu.VgsError) as e:
        eng.compare_labels(ref)
    assert e.value.status == lib.VGS_E_STATE
    eng.set_points(xyz)
    eng.voxelize(); eng.features(); eng.adjacency()
    with pytest.raises(gpu.VgsError) as e:
        eng.compare_labels(ref)
    assert e.value.status == lib.VGS_E_STATE
    assert _raw_get(eng) == lib.VGS_E_STATE
    eng.segment()
    assert _raw_get(eng) == lib.VGS_E_STATE and b"vgs_compare_labels" in eng._L.vgs_last_error_string(eng._h)   # segmented, no compare yet
    with pytest.raises(gpu.VgsError) as e:
        eng.label_comparison_device()
    assert e.value.status == lib.VGS_E_STATE
    for bad in (ref[:-1], np.concatenate([ref, ref[:1]])):
        with pytest.raises(gpu.VgsError) as e:
            eng.compare_labels(bad)
        assert e.value.status == lib.VGS_E_ARG and "n =" in str(e.value)
    assert eng._L.vgs_compare_labels(eng._h, None, N, None, None, None) == lib.VGS_E_ARG
    assert b"ref" in eng._L.vgs_last_error_string(eng._h)
    assert _raw_get(eng) == lib.VGS_E_STATE                                                   # a refused compare leaves none behind
    torch = pytest.importorskip("torch")
    with pytest.raises(gpu.VgsError) as e:
        eng.compare_labels(torch.zeros(N - 1, dtype=torch.int32, device="cuda:0"))
    assert e.value.status == lib.VGS_E_ARG
    assert eng._L.vgs_compare_labels(eng._h, ref.ctypes.data_as(C.c_void_p), N, None, None, None) == lib.VGS_OK     # every output NULL
    assert _raw_get(eng) == lib.VGS_OK
    got = eng.compare_labels(ref)
    assert R.same(got, R.compare_labels(eng.point_labels(), ref, eng.counts()["kept"]))
    # a later set_points / run invalidates the comparison
    eng.set_points(xyz)
    assert _raw_get(eng) == lib.VGS_E_STATE
    with pytest.raises(gpu.VgsError) as e:
        eng.compare_labels(ref)
    assert e.value.status == lib.VGS_E_STATE
    eng.run()
    assert _raw_get(eng) == lib.VGS_E_STATE
    assert R.same(eng.compare_labels(ref), got)


def test_empty_frames_never_show_the_previous_comparison(gpu):
    xyz = gpu.scenes.town_scene(60_000)
    N = xyz.shape[0]
    ref = (np.arange(N) % 11).astype(np.int32)
    eng = _engine(gpu, xyz)
    assert eng.compare_labels(ref)["summary"][4] > 0
    # no annotated point: empty cells and ids, the K segment rows empty, only summary[1] counts
    none = eng.compare_labels(np.full(N, -1, np.int32))
    assert R.same(none, R.compare_labels(eng.point_labels(), np.full(N, -1, np.int32), eng.counts()["kept"]))
    assert none["summary"].tolist() == [0, N] + [0] * 10
    # no kept segment: every annotated point is dropped
    e0 = _engine(gpu, xyz, voxels_min=10_000_000)
    assert e0.counts()["kept"] == 0
    k0 = e0.compare_labels(ref)
    assert R.same(k0, R.compare_labels(e0.point_labels(), ref, 0))
    assert k0["seg_annotated"].shape == (0,) and k0["summary"][2] == N and (k0["ref_best_seg"] == -1).all() and not k0["summary"][5:8].any()
    # no point at all, on the context that has just compared 60 000
    eng.set_points(np.zeros((0, 3), np.float32))
    eng.run()
    z = eng.compare_labels(np.zeros(0, np.int32))
    assert not z["summary"].any() and all(z[n].size == 0 for n, _, _ in gpu.Engine.COMPARE_FIELDS)
    assert _raw_get(eng) == gpu._lib.VGS_OK


def test_tile_context_is_refused(gpu):
    xyz = gpu.scenes.town_scene(60_000)
    eng = gpu.Engine(gpu.default_params(2))
    eng.set_points(xyz)
    lo = np.array([-1e9, -1e9], dtype=np.float64)
    hi = np.array([1e9, 1e9], dtype=np.float64)
    eng._ck(eng._L.vgs_set_owned_region(eng._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    eng.run()
    with pytest.raises(gpu.VgsError) as e:
        eng.compare_labels(np.zeros(xyz.shape[0], np.int32))
    assert e.value.status == gpu._lib.VGS_E_STATE and "tile context" in str(e.value)


def test_reused_context_reports_the_second_cloud(gpu):
    xyz1, xyz2 = gpu.scenes.town_scene(60_000), gpu.scenes.urban_scene(40_000)
    eng = _engine(gpu, xyz1)
    r1 = (np.arange(xyz1.shape[0]) % 300).astype(np.int32)
    first = eng.compare_labels(r1)
    eng.set_points(xyz2)
    eng.run()
    lab2, K2 = eng.point_labels(), eng.counts()["kept"]
    for r2 in (_labellings(lab2, K2)["structured"], (np.arange(xyz2.shape[0]) % 7 - 1).astype(np.int32)):
        got = eng.compare_labels(r2)
        assert R.same(got, R.compare_labels(lab2, r2, K2)), R.diff(got, R.compare_labels(lab2, r2, K2))
        assert R.same(got, _engine(gpu, xyz2).compare_labels(r2))          # what a fresh context gives
    assert first["summary"][0] == xyz1.shape[0] != got["summary"][0] + got["summary"][1]


# ---------------------------------------------------------------- 6. the C++ mirror and vgs_run
def test_vgs_run_csvs_and_class_mirror_round_trip(gpu, tmp_path):
    from test_cpp_segment_desc import RUN, VGS_LINES, _class_run, _write_task
    xyz = gpu.scenes.town_scene(60_000)
    N = xyz.shape[0]
    eng = _engine(gpu, xyz)
    truth = _labellings(eng.point_labels(), eng.counts()["kept"])["structured"].astype(np.int64)
    truth = np.where(truth >= 0, truth + (1 << 24) + 1, truth).astype(np.int32)     # ids a float field could not carry
    truth[::97] = -1
    want = eng.compare_labels(truth)
    gpu.pcd.write_pcd(tmp_path / "in.pcd", xyz, mode="binary", extra={"instance": truth})
    lines = dict(VGS_LINES)
    lines.update({12: str(tmp_path) + "/", 15: "in.pcd", 18: str(tmp_path) + "/", 21: "out.pcd"})
    _write_task(tmp_path / "task.txt", 2, lines)
    seg_csv, ref_csv = tmp_path / "seg.csv", tmp_path / "truth.csv"
    out = subprocess.run([RUN, str(tmp_path / "task.txt"), "--segment-matches", str(seg_csv), "--truth-field", "instance", "--truth-matches", str(ref_csv)],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    with open(seg_csv) as f:
        assert f.readline().strip() == "label,n_annotated,n_refs,best_ref,best_n,best_iou"
    rows = np.loadtxt(seg_csv, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    K = want["seg_annotated"].size
    assert rows.shape == (K, 6) and np.array_equal(rows[:, 0], np.arange(K))
    for col, name in enumerate(("seg_annotated", "seg_refs", "seg_best_ref", "seg_best_n"), 1):
        assert np.array_equal(rows[:, col].astype(np.int64), want[name]), name
    assert np.array_equal(rows[:, 5], want["seg_best_iou"])                      # %.17g reads back exactly
    with open(ref_csv) as f:
        assert f.readline().strip() == "ref_id,n_points,n_dropped,best_seg,best_n,best_iou"
    rows = np.loadtxt(ref_csv, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    assert rows.shape == (want["ref_id"].size, 6)
    for col, name in enumerate(("ref_id", "ref_points", "ref_dropped", "ref_best_seg", "ref_best_n")):
        assert np.array_equal(rows[:, col].astype(np.int64), want[name]), name
    assert np.array_equal(rows[:, 5], want["ref_best_iou"])
    assert len(out) == 3 and out[1].split()[0] == "matches" and out[2].split()[0] == "scores"
    assert [int(v) for v in out[1].split()[1:]] == want["summary"].tolist()
    sc = gpu.comparison_scores(want, 0.5)
    vals = out[2].split()[1:]
    assert int(vals[0]) == sc["matched"] > 0
    for v, key in zip(vals[1:], ("precision", "recall", "f1", "purity", "completeness", "ari")):
        assert R.close(float(v), sc[key]), (key, v, sc[key])
    # a field that is not integral ends the run instead of being rounded
    r = subprocess.run([RUN, str(tmp_path / "task.txt"), "--segment-matches", str(tmp_path / "no.csv"), "--truth-field", "x"], capture_output=True)
    assert r.returncode == 1 and b"not an integer" in r.stderr
    # the Python mirror of the classes: empty before drawColorMapofPointsinClusters, the engine's tables afterwards
    v = gpu.VoxelBasedSegmentation(0.15)
    v.setInputCloud(xyz); v.getCloudPointNum(xyz); v.addPointsFromInputCloud()
    v.setVoxelSize(0.15, 10, 3, 3)
    v.setVoxelCenters(); v.calcualteVoxelCloudAttributes(xyz); v.findAllVoxelAdjacency(0.5)
    v.segmentVoxelCloudWithGraphModel(0.3, 0.2, 0.2, 0.2, 0.2, 0.2, 2.0)
    e = v.compareClusterLabels(truth)
    assert not e["summary"].any() and all(e[n].size == 0 for n, _, _ in gpu.Engine.COMPARE_FIELDS)
    v.drawColorMapofPointsinClusters()
    assert R.same(v.compareClusterLabels(truth), want)
    s = _class_run(gpu, 3, xyz)
    assert R.same(s.compareClusterLabels(truth), s.engine.compare_labels(truth))
