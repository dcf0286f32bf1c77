"""Tables of any per-point labelling across the ranks of the native tiled driver (vgs_tiles_point_label_descriptors, _boxes and
vgs_tiles_compare_point_labels, include/vgs_tiles.h), ranks as threads of this process over LocalGroup on one GPU.  Every rank hands in the
labels of its own points only; only per-label records cross.  The reference is ONE plain engine over the gathered points in rank order
(its grid is the shared grid, as test_gpu_tiles_segdesc.py relies on): integer fields, exact boxes and the comparison by bytes, the fp64
fields against helpers.ref_descriptors within the tolerances of test_gpu_point_label_tables._check_rows, the extents against
segment_boxes_ref.ref_boxes with ==.
  * 2x1 and 2x2 layouts of scenes.tiled_urban_scene and 2x2 far from the origin, a labelling that alternates inside voxels;
  * one rank: a plain engine's tables byte for byte;
  * the driver's own labels and its refined labels;
  * designed scenes at the chunk and fold limits, with voxels that two and four ranks share;
  * call order and side effects; the status contract; the front end."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import label_compare_ref as R
from segment_scenes import BIG_NODES, FAR, GROUP, big_nodes
from test_gpu_point_label_tables import BOX, DESC, FRAMES, _check_rows
from test_gpu_segment_boxes import _check_frame
from test_gpu_segment_limits import _split
from test_gpu_tiles_segdesc import _parts, _pitch, _ranks, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")
N_PER = 60_000
SD_CHUNK = 2048
INTS = ("n_points", "n_nodes", "bbox6")


class _Tables:
    """the tiled tables behind the interface _check_rows reads, with the reference engine's voxels"""

    def __init__(self, eng, d, boxes):
        self.eng, self.d, self.boxes = eng, d, boxes

    def describe_labels(self, labels, K=None):
        return self.d

    def label_boxes(self, labels, frame="principal", K=None):
        return self.boxes[frame]

    def point_voxel(self):
        return self.eng.point_voxel()


def _engine(gpu, xyz, params=None):
    eng = gpu.Engine(params if params is not None else gpu.default_params(2, voxel_size=0.1))
    eng.set_points(xyz)
    eng.run()
    return eng


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)


def _tables(t, lab, K, ref):
    return dict(d=t.describe_labels(lab, K), b={f: t.label_boxes(lab, f, K) for f in FRAMES}, c=t.compare_labels(ref, labels=lab, K=K))


def _same_tables(a, b):
    da = {k: v for k, v in a["d"].items() if k != "n_skipped"}
    db = {k: v for k, v in b["d"].items() if k != "n_skipped"}
    return (_same(da, db) and a["d"]["n_skipped"] == b["d"]["n_skipped"] and all(_same(a["b"][f], b["b"][f]) for f in FRAMES) and
            R.same(a["c"], b["c"]) and np.array_equal(a["c"]["summary"], b["c"]["summary"]))


def _against_engine(eng, xyz, lab, K, ref, got):
    """the tiled tables `got` of the labelling `lab` of the gathered points against the plain engine over them"""
    want = eng.describe_labels(lab, K=K)
    for name in INTS:
        assert got["d"][name].tobytes() == want[name].tobytes() and got["d"][name].dtype == want[name].dtype, name
    assert got["d"]["n_skipped"] == want["n_skipped"]
    wc = eng.compare_labels(ref, labels=lab, K=K)
    assert R.same(got["c"], wc), R.diff(got["c"], wc)
    assert np.array_equal(got["c"]["summary"], wc["summary"])
    # (_check_rows indexes a table by the labels: every negative label is handed to it as -1, the row they all mean)
    _check_rows(_Tables(eng, got["d"], got["b"]), xyz, np.where(lab < 0, -1, lab).astype(np.int32), K)
    for f in FRAMES:
        _check_frame(got["b"][f], got["d"], f)


# ---------------------------------------------------------------- 1. layouts
def _mixed_labels(point_labels, first, n_bad):
    """(point_label * 2 + i % 2) over the gathered index i = first + j: two labels inside every voxel of a segment; some points negative;
    the rank's last n_bad points (not finite) carry a label all the same"""
    i = first + np.arange(point_labels.shape[0], dtype=np.int64)
    lab = np.where(point_labels >= 0, point_labels.astype(np.int64) * 2 + i % 2, -1)
    lab[i % 17 == 3] = -5
    if n_bad:
        lab[-n_bad:] = 1
    return np.ascontiguousarray(lab.astype(np.int32))


def _ref_ids(first, n):
    i = first + np.arange(n, dtype=np.int64)
    return np.ascontiguousarray((i // 97 % 23 - 1).astype(np.int32))


@pytest.mark.parametrize("layout", ["2x1", "2x2", "2x2_far"])
def test_layouts_match_one_engine_over_the_gathered_points(gpu, layout):
    tiles = (2, 1) if layout == "2x1" else (2, 2)
    shift = FAR if layout.endswith("far") else None
    parts = _parts(gpu, tiles, n_per=N_PER, shift=shift)
    bad = np.array([[np.nan, 1.0, 1.0]], np.float32)
    parts = [np.concatenate([p, bad]) for p in parts]   # one point per rank outside the octree, labelled below
    off = _offsets(parts)

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        pl, kept = t.point_labels()
        K = 2 * kept + 3
        lab, ref = _mixed_labels(pl, off[r], 1), _ref_ids(off[r], xyz.shape[0])
        first = _tables(t, lab, K, ref)
        second = _same_tables(_tables(t, lab, K, ref), first)
        t.run()
        rerun = _same_tables(_tables(t, lab, K, ref), first)
        times = t.point_label_times()
        t.describe_labels(lab, K)   # (the payload of a box call holds extent entries too, whose number this rank's tables do not tell)
        return dict(kept=kept, K=K, lab=lab, ref=ref, t=first, second=second, rerun=rerun, pay=t.point_label_payload(), times=times)
    out = _ranks(gpu, tiles, _pitch(N_PER), parts, body, center=shift[:2] if shift else (0.0, 0.0))
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    K = out[0]["K"]
    for o in out:
        assert o["K"] == K and _same_tables(o["t"], out[0]["t"]) and o["second"] and o["rerun"]
        assert o["times"]["total"] > 0
        # the wire size of the descriptor call: 128-byte entries -- the header, the moment records, the pair records eight to an entry
        assert o["pay"]["bytes_sent"] == 128 * (1 + o["pay"]["own_records"] + -(-o["pay"]["own_pairs"] // 8)), o["pay"]
    xyz = np.concatenate(parts)
    lab, ref = np.concatenate([o["lab"] for o in out]), np.concatenate([o["ref"] for o in out])
    eng = _engine(gpu, xyz)
    got = out[0]["t"]
    assert got["d"]["n_skipped"] == len(parts)
    assert (got["d"]["n_points"][-3:] == 0).all()          # three labels no point carries anywhere
    _against_engine(eng, xyz, lab, K, ref, got)
    rank_of = np.repeat(np.arange(len(parts)), [p.shape[0] for p in parts])
    on = np.zeros((K, len(parts)), bool)
    on[lab[lab >= 0], rank_of[lab >= 0]] = True
    assert (on.sum(axis=1) >= 2).any()                      # a checked label has points on two ranks
    assert sum(o["pay"]["own_pairs"] for o in out) > 0      # and voxels that two ranks share


# ---------------------------------------------------------------- 2. one rank
def test_one_rank_equals_a_plain_engine(gpu):
    xyz = gpu.scenes.urban_scene(120_000)

    def body(r, t, p):
        t.set_points(p)
        t.run()
        pl, kept = t.point_labels()
        K = 2 * kept + 3
        lab = _mixed_labels(pl, 0, 0)
        ref = _ref_ids(0, p.shape[0])
        host = _tables(t, lab, K, ref)
        dev = _tables(t, torch.from_numpy(lab).to("cuda:0"), K, torch.from_numpy(ref).to("cuda:0"))   # read in place on the device
        return dict(K=K, lab=lab, t=host, device=_same_tables(dev, host))
    torch = pytest.importorskip("torch")
    o = _ranks(gpu, (1, 1), 1000.0, [xyz], body)[0]
    assert not isinstance(o, Exception), o
    assert o["device"]
    eng = _engine(gpu, xyz)
    K, lab = o["K"], o["lab"]
    want = eng.describe_labels(lab, K=K)
    for name in DESC:
        assert o["t"]["d"][name].tobytes() == want[name].tobytes(), name
    assert o["t"]["d"]["n_skipped"] == want["n_skipped"]
    for f in FRAMES:
        wb = eng.label_boxes(lab, f, K=K)
        for name in BOX:
            assert o["t"]["b"][f][name].tobytes() == wb[name].tobytes(), (f, name)
    wc = eng.compare_labels(_ref_ids(0, xyz.shape[0]), labels=lab, K=K)
    assert R.same(o["t"]["c"], wc) and np.array_equal(o["t"]["c"]["summary"], wc["summary"])


# ---------------------------------------------------------------- 3. and 5. the driver's own labels; call order and side effects
def test_the_drivers_own_labels_refined_labels_and_side_effects(gpu):
    """Handed point_labels(), the integer fields and the boxes' input equal the cached segment_descriptors() by bytes.  The fp64 fields
    agree within the tolerances of _check_rows only: the cached pass chunks a segment's points node by node in sorted-node order and
    filters the own ones inside each chunk, this pass chunks the own points alone, so the fixed summation shapes differ."""
    tiles = (2, 1)
    parts = _parts(gpu, tiles, n_per=N_PER)
    off = _offsets(parts)

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        pl, kept = t.point_labels()
        ref = _ref_ids(off[r], xyz.shape[0])
        cached = dict(d=t.segment_descriptors(), b={f: t.segment_boxes(f) for f in FRAMES}, g=t.segment_graph())
        counts = t.refine_labels()
        refined = t.refined_labels().copy()
        plain_cmp = t.compare_labels(ref)
        ex0 = t.exchange()
        # boxes before descriptors, the other frame afterwards: not a byte changes
        b0 = t.label_boxes(pl, "upright", kept)
        d0 = t.describe_labels(pl, kept)
        b1 = t.label_boxes(pl, "principal", kept)
        own = _tables(t, pl, kept, ref)
        order = _same(b0, own["b"]["upright"]) and _same(b1, own["b"]["principal"]) and all(d0[n].tobytes() == own["d"][n].tobytes() for n in DESC)
        ref_t = _tables(t, refined, kept, ref)
        pl2, _ = t.point_labels()
        untouched = (np.array_equal(pl, pl2) and _same(cached["d"], t.segment_descriptors()) and _same(cached["g"], t.segment_graph()) and
                     all(_same(cached["b"][f], t.segment_boxes(f)) for f in FRAMES) and np.array_equal(refined, t.refined_labels()) and
                     t.exchange() == ex0)
        return dict(kept=kept, pl=pl, ref=ref, cached=cached, own=own, order=order, refined=refined, ref_t=ref_t, untouched=untouched,
                    plain_cmp=plain_cmp, counts=counts)
    out = _ranks(gpu, tiles, _pitch(N_PER), parts, body)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    kept = out[0]["kept"]
    for o in out:
        assert o["order"] and o["untouched"]
        assert _same_tables(o["own"], out[0]["own"]) and _same_tables(o["ref_t"], out[0]["ref_t"])
    own, cached = out[0]["own"], out[0]["cached"]
    for name in INTS:
        assert own["d"][name].tobytes() == cached["d"][name].tobytes(), name
    assert R.same(own["c"], out[0]["plain_cmp"]) and np.array_equal(own["c"]["summary"], out[0]["plain_cmp"]["summary"])
    a, b = own["d"], cached["d"]
    assert (np.abs(a["centroid3"] - b["centroid3"]) <= 1e-9 * (1 + np.linalg.norm(b["centroid3"], axis=1))[:, None]).all()
    tr = b["cov6"][:, [0, 3, 5]].sum(axis=1)
    assert (np.abs(a["cov6"] - b["cov6"]) <= 1e-8 * tr[:, None] + 1e-30).all()
    assert (np.abs(a["evals3"] - b["evals3"]) <= 1e-8 * b["evals3"][:, 2:3] + 1e-30).all()
    xyz = np.concatenate(parts)
    eng = _engine(gpu, xyz)
    pl, ref = np.concatenate([o["pl"] for o in out]), np.concatenate([o["ref"] for o in out])
    _against_engine(eng, xyz, pl, kept, ref, own)
    refined = np.concatenate([o["refined"] for o in out])
    assert sum(o["counts"]["points_filled"] + o["counts"]["points_changed"] for o in out) > 0 and not np.array_equal(refined, pl)
    _against_engine(eng, xyz, refined, kept, ref, out[0]["ref_t"])


# ---------------------------------------------------------------- 4. structural limits on designed scenes
CENTER = (0.05, 22.55)                  # x through the middle of every group's first voxel, y through the middle of a voxel row
SIZES = (SD_CHUNK - 1, SD_CHUNK, SD_CHUNK + 1, 2 * SD_CHUNK + 1, 64 * SD_CHUNK + 1)   # a chunk, its neighbours, three chunks, the fold's lane stride
FILL = ((-5.0, 10.0), (5.0, 10.0), (-5.0, 35.0), (5.0, 35.0))    # a slab of points deep inside every rank's region
K_DESIGNED = 40


def _designed_scene():
    rng = np.random.default_rng(3)
    corner = np.array([CENTER[0], CENTER[1], 0.05]) + rng.uniform(-0.002, 0.002, (4000, 3))   # one voxel, four ranks
    n_fill = sum(SIZES) + 50
    fill = [np.array([x, y, 0.02]) + rng.uniform(-0.5, 0.5, (n_fill, 3)) * [1.0, 1.0, 0.04] for x, y in FILL]
    return np.concatenate([big_nodes(), corner] + fill).astype(np.float32)


def _designed_labels(parts, variant):
    """per rank the labels of its own points: 0 .. 8 the shared-voxel cases, 10 + 5 r + s the label of SIZES[s] points on rank r alone"""
    labs = []
    for r, p in enumerate(parts):
        n = p.shape[0]
        j = np.arange(n)
        lab = np.full(n, -1, np.int64)
        left = r % 2 == 0
        vox0 = np.abs(p[:, 0] - 0.05) < 0.01                      # the straddling first voxel of a group (or the corner voxel)
        grp = lambda g: vox0 & (np.abs(p[:, 1] - ((g + 1) * 3.0 + 0.05)) < 0.01)   # noqa: E731
        lab[grp(5)] = 0                                            # both sides give label 0: counted once
        lab[grp(4)] = 1 if left else 2                             # the sides give 1 and 2: one each
        lab[grp(3)] = np.where(j % 2 == 0, 3, 4)[grp(3)] if left else 3   # one side alternates 3 / 4 inside the voxel
        lab[grp(8)] = -1 if left else 5                            # one side is all negative
        corner = vox0 & (np.abs(p[:, 1] - CENTER[1]) < 0.01)
        assert corner.sum() > 500
        lab[corner] = (6, 6, -1, -3)[r]
        if r == 2:
            lab[corner] = np.where(j % 2 == 0, 6, 7)[corner]
        fill = np.flatnonzero((np.abs(p[:, 0] - FILL[r][0]) < 0.6) & (np.abs(p[:, 1] - FILL[r][1]) < 0.6))
        at = 0
        for s, size in enumerate(SIZES):
            lab[fill[at:at + size]] = 10 + 5 * r + s
            at += size
        if r < 2:
            lab[fill[at]] = 8                                      # one point on each of two ranks
        if variant == "rank3_negative" and r == 3:
            lab[:] = -2
        if variant == "K1":
            lab = np.where(lab >= 0, 0, lab)
        if variant == "K0":
            lab[:] = -1
        labs.append(np.ascontiguousarray(lab.astype(np.int32)))
    return labs


VARIANTS = {"main": K_DESIGNED, "rank3_negative": K_DESIGNED, "K1": 1, "K0": 0}


def test_structural_limits_and_shared_voxels_on_designed_scenes(gpu):
    from vgs_svgs_segmentation_amd import tiles_native as tn
    params = gpu.default_params(2, **GROUP)
    xyz = _designed_scene()
    parts = _split(xyz, CENTER)
    labs = {v: _designed_labels(parts, v) for v in VARIANTS}
    off = _offsets(parts)

    def body(r, t, p):
        t.set_points(p)
        t.run()
        res = {}
        for v, K in VARIANTS.items():
            lab = labs[v][r]
            tab = _tables(t, lab, K, _ref_ids(off[r], p.shape[0]))
            res[v] = dict(t=tab, pay=t.point_label_payload(), own=t.own_point_label_moments(K, lab))
        return res
    out = _ranks(gpu, (2, 2), 50.0, parts, body, center=CENTER, params=params)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    all_xyz = np.concatenate(parts)
    eng = _engine(gpu, all_xyz, params)
    pv = eng.point_voxel().astype(np.int64)
    rank_of = np.repeat(np.arange(4), [p.shape[0] for p in parts])
    ranks_in_voxel = np.zeros((int(pv.max()) + 1, 4), bool)
    ranks_in_voxel[pv[pv >= 0], rank_of[pv >= 0]] = True
    n_ranks = ranks_in_voxel.sum(axis=1)
    assert (n_ranks == 4).sum() == 1 and (n_ranks == 2).sum() >= len(BIG_NODES)     # the corner voxel; the groups' first voxels
    assert np.bincount(pv[pv >= 0])[n_ranks >= 2].max() > SD_CHUNK                   # a straddling voxel larger than a chunk
    ref = _ref_ids(0, all_xyz.shape[0])
    for v, K in VARIANTS.items():
        lab = np.concatenate(labs[v])
        got = out[0][v]["t"]
        for o in out:
            assert _same_tables(o[v]["t"], got), v
        if K == 0:
            assert got["d"]["n_points"].shape == (0,) and got["b"]["principal"]["lo3"].shape == (0, 3) and got["d"]["n_skipped"] == 0
            assert R.same(got["c"], R.compare_labels(lab, ref, 0))
            continue
        _against_engine(eng, all_xyz, lab, K, ref, got)
        for r, o in enumerate(out):
            mine = (rank_of == r) & (lab >= 0) & (pv >= 0)
            shared = mine & (n_ranks[np.maximum(pv, 0)] >= 2)
            want_pairs = np.unique(pv[shared] * K + lab[shared]).size
            assert o[v]["pay"]["own_pairs"] == want_pairs == o[v]["own"]["pair_label"].size, (v, r)
            assert o[v]["pay"]["own_records"] == np.unique(lab[mine]).size == o[v]["own"]["label"].size, (v, r)
        folded = tn.fold_moments([o[v]["own"] for o in out], K)
        add = tn.fold_label_pairs([o[v]["own"] for o in out], K)
        assert np.array_equal(folded["n_points"], got["d"]["n_points"]) and np.array_equal(folded["n_nodes"] + add, got["d"]["n_nodes"])
        assert folded["bbox6"].tobytes() == got["d"]["bbox6"].tobytes()
    main = out[0]["main"]["t"]["d"]
    for r in range(4):
        assert main["n_points"][10 + 5 * r:15 + 5 * r].tolist() == list(SIZES)
    assert main["n_nodes"][[0, 1, 2, 3, 4, 5, 6, 7]].tolist() == [1] * 8 and main["n_points"][8] == 2 and main["n_nodes"][8] == 2
    assert main["n_points"][9] == 0 and (main["n_points"][30:] == 0).all()
    assert out[3]["rank3_negative"]["pay"]["own_records"] == 0 and out[3]["rank3_negative"]["pay"]["own_pairs"] == 0


# ---------------------------------------------------------------- 6. the status contract
def test_before_a_run_is_refused_without_a_collective(gpu):
    from vgs_svgs_segmentation_amd import tiles_native as tn
    grp = tn.LocalGroup(2)
    t = tn.NativeTiles(gpu.default_params(2, voxel_size=0.1), tn.COMM_LOCAL, grp.handle, 0, 2, (2, 1), 5.0)
    lab = np.zeros(4, np.int32)
    try:
        for call in (lambda: t.describe_labels(lab, 3), lambda: t.label_boxes(lab, "upright", 3), lambda: t.compare_labels(lab, labels=lab, K=3)):
            with pytest.raises(gpu.VgsError, match="VGS_E_STATE"):
                call()   # rank 0 alone comes back: no collective
    finally:
        t.close()
        grp.close()


def test_failures_travel_in_the_status_word(gpu):
    parts = _parts(gpu, (2, 1), n_per=20_000)

    def attempt(call):
        try:
            call()
            return "finished"
        except Exception as ex:  # noqa: BLE001
            return ex

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        n = xyz.shape[0]
        good = np.zeros(n, np.int32)
        bad = good.copy()
        if r == 1:
            bad[[700, 311]] = 3
        ref = np.zeros(n, np.int32)
        res = {}
        res["label"] = attempt(lambda: t.describe_labels(bad, 3))
        res["label_boxes"] = attempt(lambda: t.label_boxes(bad, "upright", 3))
        res["label_compare"] = attempt(lambda: t.compare_labels(ref, labels=bad, K=3))
        res["n"] = attempt(lambda: t.describe_labels(good[:-1] if r == 1 else good, 3))
        res["frame"] = attempt(lambda: t.label_boxes(good, 2 if r == 1 else 1, 3))
        res["K"] = attempt(lambda: t.describe_labels(good, 3 + r))
        res["K_compare"] = attempt(lambda: t.compare_labels(ref, labels=good, K=3 + r))
        res["after"] = attempt(lambda: t.describe_labels(good, 3))   # the driver is usable after all of them
        L = gpu._lib.lib()
        st = L.vgs_point_label_descriptors(t._ctx(), good.ctypes.data_as(C.c_void_p), n, 3, *([None] * 9))
        res["single"] = (st, L.vgs_last_error_string(t._ctx()).decode())
        return res
    out = _ranks(gpu, (2, 1), _pitch(20_000), parts, body, timeout=120.0)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    E = gpu.VgsError
    for case in ("label", "label_boxes", "label_compare"):
        assert isinstance(out[1][case], E) and "VGS_E_ARG" in str(out[1][case]) and "[311] = 3" in str(out[1][case]), (case, out[1][case])
        assert isinstance(out[0][case], E) and "VGS_E_PEER" in str(out[0][case]) and "rank 1" in str(out[0][case]), (case, out[0][case])
    for case in ("n", "frame"):
        assert isinstance(out[1][case], E) and "VGS_E_ARG" in str(out[1][case]), (case, out[1][case])
        assert isinstance(out[0][case], E) and "VGS_E_PEER" in str(out[0][case]) and "rank 1" in str(out[0][case]), (case, out[0][case])
    for case in ("K", "K_compare"):
        for o in out:
            assert isinstance(o[case], E) and "VGS_E_ARG" in str(o[case]) and "rank 1 passed K = 4" in str(o[case]), (case, o[case])
    for o in out:
        assert o["after"] == "finished", o["after"]
        assert o["single"][0] == gpu._lib.VGS_E_STATE and "tile context" in o["single"][1]


def test_an_injected_failure_takes_the_peer_out(gpu, monkeypatch):
    monkeypatch.setenv("VGS_TILES_FAIL_RANK", "1")
    monkeypatch.setenv("VGS_TILES_FAIL_AT", "point_labels")
    parts = _parts(gpu, (2, 1), n_per=20_000)

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        t.describe_labels(np.zeros(xyz.shape[0], np.int32), 2)
        return "finished"
    out = _ranks(gpu, (2, 1), _pitch(20_000), parts, body, timeout=120.0)
    assert isinstance(out[1], gpu.VgsError) and "VGS_E_STATE" in str(out[1]) and "point_labels" in str(out[1]), out[1]
    assert isinstance(out[0], gpu.VgsError) and "VGS_E_PEER" in str(out[0]) and "rank 1" in str(out[0]), out[0]


# ---------------------------------------------------------------- 7. the front end
def test_tiles_run_front_end_writes_the_refined_tables(gpu, tmp_path):
    tiles = (2, 1)
    parts = _parts(gpu, tiles, n_per=N_PER)
    off = _offsets(parts)
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    prefix = str(tmp_path / "t")
    for r, p in enumerate(parts):
        np.ascontiguousarray(p, dtype=np.float32).tofile(f"{prefix}.{r}.f32")
        _ref_ids(off[r], p.shape[0]).tofile(f"{prefix}.{r}.truth.i32")
    seg, box, mat, tru = (str(tmp_path / n) for n in ("seg.csv", "box.csv", "mat.csv", "tru.csv"))
    text = subprocess.check_output([EXE, "--emulate", "2x1", "--pitch", repr(float(_pitch(N_PER))), "--voxel", "0.1", "--refine", "--refined-segments", seg,
                                    "--refined-segment-boxes", box, "--box-frame", "upright", "--refined-matches", mat, "--refined-truth-matches", tru,
                                    prefix], text=True, timeout=300)
    kept = int(text.strip().splitlines()[0].split()[1])

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        _, k = t.point_labels()
        t.refine_labels()
        fine = t.refined_labels().copy()
        return dict(kept=k, fine=fine, d=t.describe_labels(fine, k), b=t.label_boxes(fine, "upright", k),
                    c=t.compare_labels(_ref_ids(off[r], xyz.shape[0]), labels=fine, K=k))
    o = _ranks(gpu, tiles, _pitch(N_PER), parts, body)[0]
    assert not isinstance(o, Exception), o
    assert o["kept"] == kept
    assert np.array_equal(np.fromfile(f"{prefix}.0.refined.i32", dtype=np.int32), o["fine"])   # the labels the tables describe
    d, b, w = o["d"], o["b"], o["c"]
    rows = np.loadtxt(seg, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    assert rows.shape == (kept, 29) and np.array_equal(rows[:, 0], np.arange(kept))
    assert np.array_equal(rows[:, 1].astype(np.int64), d["n_points"]) and np.array_equal(rows[:, 2].astype(np.int32), d["n_nodes"])
    assert np.array_equal(rows[:, 3:9].astype(np.float32), d["bbox6"])
    assert np.array_equal(rows[:, 9:12], d["centroid3"]) and np.array_equal(rows[:, 12:15], d["evals3"])
    V = d["evecs9"].reshape(kept, 3, 3)
    assert np.array_equal(rows[:, 15:18], V[:, :, 0]) and np.array_equal(rows[:, 18:21], V[:, :, 2])
    assert np.array_equal(rows[:, 21:29].astype(np.float32), d["eigen8"])
    tab = np.loadtxt(box, delimiter=",", skiprows=1, ndmin=2)
    assert tab.shape == (kept, 22)
    for name, sl in (("center3", slice(1, 4)), ("half3", slice(4, 7)), ("frame9", slice(7, 16)), ("lo3", slice(16, 19)), ("hi3", slice(19, 22))):
        assert np.array_equal(tab[:, sl], b[name]), name      # %.17g round-trips a double
    with open(mat) as f:
        assert f.readline().strip() == "label,n_annotated,n_refs,best_ref,best_n,best_iou"
    rows = np.loadtxt(mat, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    assert rows.shape == (kept, 6) and np.array_equal(rows[:, 0], np.arange(kept))
    for col, name in enumerate(("seg_annotated", "seg_refs", "seg_best_ref", "seg_best_n"), 1):
        assert np.array_equal(rows[:, col].astype(np.int64), w[name]), name
    assert np.array_equal(rows[:, 5], w["seg_best_iou"])
    rows = np.loadtxt(tru, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    assert rows.shape == (w["ref_id"].size, 6)
    for col, name in enumerate(("ref_id", "ref_points", "ref_dropped", "ref_best_seg", "ref_best_n")):
        assert np.array_equal(rows[:, col].astype(np.int64), w[name]), name
    assert np.array_equal(rows[:, 5], w["ref_best_iou"])
