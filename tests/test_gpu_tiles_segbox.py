"""Oriented bounding boxes across the ranks of the native tiled driver (vgs_tiles_get_segment_boxes, include/vgs_tiles.h), ranks as threads
of this process over LocalGroup on one GPU, in both frames:
  * 2x1, 2x2 and 4x2 layouts of scenes.tiled_urban_scene, and 2x2 far from the origin: every rank's table has the same bytes; the frames
    pass test_gpu_segment_boxes._check_frame against the tiled descriptor table (principal = evecs9 byte for byte); lo3, hi3, half3 and
    center3 equal tests/segment_boxes_ref.py over the gathered points by ==, without a tolerance; the table survives a second call and a
    second run bit for bit; neither the size query nor a cached call waits for a peer; labels, descriptors and graph are not touched;
    each rank's own records (vgs_get_own_segment_extents) name exactly the labels of its own points and fold to the table;
  * the order of the calls (boxes before descriptors, the other frame afterwards) does not change a byte;
  * one rank: equal to a plain engine's vgs_get_segment_boxes;
  * nodes larger than a chunk whose points two ranks share; degenerate segments, one-point segments on two ranks, signed zeros;
  * an injected failure in the box phase takes the peer out with it; a bad frame and a call before a run are refused without a collective;
  * examples/vgs_tiles_run --segment-boxes writes rank 0's table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from segment_boxes_ref import ref_boxes
from segment_scenes import BIG_NODES, FAR, GROUP, big_nodes, degenerate_scene
from test_gpu_segment_boxes import _check_frame
from test_gpu_segment_limits import _split
from test_gpu_tiles_segdesc import _parts, _pitch, _ranks, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")
N_PER = 60_000
FRAMES = ("principal", "upright")
EXACT = ("lo3", "hi3", "half3", "center3")
LAYOUTS = {"2x1": ((2, 1), None), "2x2": ((2, 2), None), "4x2": ((4, 2), None), "2x2_far": ((2, 2), FAR)}
_cache = {}


def _size_query(t, frame):
    K = C.c_int64(-1)
    assert t._L.vgs_tiles_get_segment_boxes(t._h, frame, C.byref(K), *([None] * 5)) == 0
    return K.value


def _collect(r, t, xyz):
    """descriptors and graph first, then both frames; again; after a second run"""
    t.set_points(xyz)
    t.run()
    labels, kept = t.point_labels()
    d, g = t.segment_descriptors(), t.segment_graph()
    first = {f: t.segment_boxes(f) for f in FRAMES}
    times = t.box_times()
    if r == 0:
        # neither the size query nor a cached call is a collective: rank 0 alone must come back
        assert all(_size_query(t, i) == kept for i in (0, 1))
        assert all(_same(t.segment_boxes(f), first[f]) for f in FRAMES)
    second = all(_same(t.segment_boxes(f), first[f]) for f in reversed(FRAMES))
    labels_after, _ = t.point_labels()
    untouched = bool(np.array_equal(labels, labels_after)) and _same(d, t.segment_descriptors()) and _same(g, t.segment_graph())
    own = {f: t.own_segment_extents(kept, f, d) for f in FRAMES}
    t.run()
    labels2, kept2 = t.point_labels()
    rerun = all(_same(t.segment_boxes(f), first[f]) for f in FRAMES)   # (boxes first this time: the descriptor collective inside)
    untouched = untouched and bool(np.array_equal(labels, labels2)) and kept2 == kept and _same(d, t.segment_descriptors())
    return dict(labels=labels, kept=kept, d=d, b=first, own=own, second=second, rerun=rerun, untouched=untouched, times=times)


def _check(parts, out, two_ranks=True):
    """the checks of the issue's "Layouts" on the results of _collect; returns (table per frame, descriptors, gathered labels)"""
    from vgs_svgs_segmentation_amd import tiles_native as tn
    world = len(parts)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    kept, d = out[0]["kept"], out[0]["d"]
    labels = np.concatenate([o["labels"] for o in out])
    xyz = np.concatenate(parts)
    assert kept > 0 and labels.max() == kept - 1
    # extents and counts cover the same points, and every row is reached
    n = np.bincount(labels[labels >= 0], minlength=kept)
    assert np.array_equal(d["n_points"], n) and (n > 0).all()
    rank_of = np.repeat(np.arange(world), [p.shape[0] for p in parts])
    lab_ranks = np.zeros((kept, world), bool)
    lab_ranks[labels[labels >= 0], rank_of[labels >= 0]] = True
    if two_ranks:
        assert (lab_ranks.sum(axis=1) >= 2).any()          # at least one checked segment has points on two ranks
    for f in FRAMES:
        b = out[0]["b"][f]
        for r, o in enumerate(out):
            assert o["kept"] == kept and _same(o["b"][f], b), (f, r)   # every rank: the same bytes
            assert o["second"] and o["rerun"] and o["untouched"], (f, r)
            assert o["times"]["total"] > 0 and o["times"]["exchange"] >= 0
        assert all(b[k].shape == (kept, w) and b[k].dtype == np.float64 for k, w in (("center3", 3), ("half3", 3), ("frame9", 9), ("lo3", 3), ("hi3", 3)))
        _check_frame(b, d, f)
        ref = ref_boxes(xyz, labels, kept, d["centroid3"], b["frame9"])
        for k in EXACT:
            bad = np.nonzero(~(b[k] == ref[k]).all(axis=1))[0]
            assert bad.size == 0, (f, k, bad[:5], b[k][bad[:5]], ref[k][bad[:5]])
        # a rank's own records: one per label with an own point there, and their fold is the table
        for r, o in enumerate(out):
            assert np.array_equal(o["own"][f]["label"], np.nonzero(lab_ranks[:, r])[0]), (f, r)
        folded = tn.fold_extents([o["own"][f] for o in out], kept)
        assert folded["reached"].all() and (folded["lo3"] == b["lo3"]).all() and (folded["hi3"] == b["hi3"]).all()
    return out[0]["b"], d, labels


def _layout(gpu, name):
    """(parts, results of _collect) of a layout, made once and shared"""
    if name not in _cache:
        tiles, shift = LAYOUTS[name]
        parts = _parts(gpu, tiles, shift=shift)
        _cache[name] = (parts, _ranks(gpu, tiles, _pitch(N_PER), parts, _collect, center=shift[:2] if shift else (0.0, 0.0)))
    return _cache[name]


# ---------------------------------------------------------------- layouts, far from the origin, counts
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_tiled_boxes_equal_the_numpy_restatement(gpu, name):
    parts, out = _layout(gpu, name)
    _check(parts, out)


# ---------------------------------------------------------------- call order
def test_call_order_does_not_change_a_byte(gpu):
    parts, base = _layout(gpu, "2x1")
    for o in base:
        assert not isinstance(o, Exception), o

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        up = t.segment_boxes("upright")          # boxes before descriptors: the descriptor collective inside the call
        d = t.segment_descriptors()
        pr = t.segment_boxes("principal")        # the other frame afterwards ...
        return dict(up=up, d=d, pr=pr, kept_up=_same(up, t.segment_boxes("upright")))   # ... leaves the first frame's table unchanged
    out = _ranks(gpu, (2, 1), _pitch(N_PER), parts, body)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
        assert o["kept_up"]
        assert _same(o["d"], base[0]["d"])
        assert _same(o["up"], base[0]["b"]["upright"]) and _same(o["pr"], base[0]["b"]["principal"])


# ---------------------------------------------------------------- one rank
def test_one_rank_equals_a_plain_engine(gpu):
    xyz = gpu.scenes.urban_scene(200_000)
    out = _ranks(gpu, (1, 1), 1000.0, [xyz],
                 lambda r, t, p: (t.set_points(p), t.run(), t.point_labels(), {f: t.segment_boxes(f) for f in FRAMES})[2:])
    assert not isinstance(out[0], Exception), out[0]
    (labels, kept), b = out[0]
    eng = gpu.Engine(gpu.default_params(2, voxel_size=0.1))
    eng.set_points(xyz)
    eng.run()
    assert np.array_equal(labels, eng.point_labels()) and kept == eng.counts()["kept"] > 0
    for f in FRAMES:
        assert _same(b[f], eng.segment_boxes(f)), f


# ---------------------------------------------------------------- structural edges
def _tiled_scene(gpu, xyz, center, pitch=50.0):
    parts = _split(xyz, center)
    assert np.array_equal(parts[0][0], xyz[0])
    out = _ranks(gpu, (2, 2), pitch, parts, _collect, center=center, params=gpu.default_params(2, **GROUP))
    return parts, out


def test_tiled_nodes_larger_than_a_chunk(gpu):
    """The split of test_gpu_segment_limits.test_tiled_nodes_larger_than_a_chunk: the border x = 0.05 m runs through the middle of every
    group's first voxel, so k_sb_chunks_own filters inside chunks that split a node of up to 10 000 points."""
    parts, out = _tiled_scene(gpu, big_nodes(), (0.05, 22.5))
    b, d, labels = _check(parts, out)
    assert sorted(d["n_points"].tolist()) == sorted([1] + [sum(g) for g in BIG_NODES])   # one segment per group
    rank_of = np.repeat(np.arange(4), [p.shape[0] for p in parts])
    big = np.nonzero((d["n_points"] == 10_000) & (d["n_nodes"] == 1))[0]
    assert big.size == 1
    assert np.unique(rank_of[labels == big[0]]).size == 2   # the 10 000-point node lies on two ranks


def test_tiled_degenerate_segments(gpu):
    """degenerate_scene() and a copy of it 8 m further in y (exact in float32), so that the scene's one-point segment exists on both sides
    of the border y = 4; the border x = 0.1 cuts the signed-zeros group.  One-point segments: lo = hi = half = 0 and the centre is the
    point; zeros of either sign compare by value."""
    base, first = degenerate_scene()
    xyz = np.concatenate([base, (base.astype(np.float64) + [0.0, 8.0, 0.0]).astype(np.float32)])
    parts, out = _tiled_scene(gpu, xyz, (0.1, 4.0))
    b, d, labels = _check(parts, out)
    rank_of = np.repeat(np.arange(4), [p.shape[0] for p in parts])
    pts = np.concatenate(parts)
    one = np.nonzero(d["n_points"] == 1)[0]
    assert np.unique(rank_of[np.isin(labels, one)]).size >= 2          # one-point segments on at least two ranks
    zeros = labels[0]                                                  # the signed-zeros group: the scene's first point, rank 0's first
    assert np.unique(rank_of[labels == zeros]).size == 2
    for f in FRAMES:
        for k in one.tolist():
            p = pts[labels == k][0].astype(np.float64)
            assert (b[f]["lo3"][k] == 0).all() and (b[f]["hi3"][k] == 0).all() and (b[f]["half3"][k] == 0).all()
            assert (b[f]["center3"][k] == p).all()
    same = d["n_points"] == 7                                          # seven points in one place: a box of no size as well
    assert same.sum() == 2 and all((b[f]["half3"][same] == 0).all() for f in FRAMES)


# ---------------------------------------------------------------- failures
def test_a_failing_rank_in_the_box_phase_takes_its_peer_out(gpu, monkeypatch):
    monkeypatch.setenv("VGS_TILES_FAIL_RANK", "1")
    monkeypatch.setenv("VGS_TILES_FAIL_AT", "boxes")
    parts = _parts(gpu, (2, 1))

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        t.segment_boxes("principal")
        return "finished"
    out = _ranks(gpu, (2, 1), _pitch(N_PER), parts, body, timeout=120.0)
    assert isinstance(out[1], gpu.VgsError) and "VGS_E_STATE" in str(out[1]) and "boxes" in str(out[1]), out[1]
    assert isinstance(out[0], gpu.VgsError) and "VGS_E_PEER" in str(out[0]) and "rank 1" in str(out[0]), out[0]


def test_bad_calls_are_refused_without_a_collective(gpu):
    """one rank of two, whose peer never calls: both errors come back, so both are decided locally"""
    from vgs_svgs_segmentation_amd import tiles_native as tn
    grp = tn.LocalGroup(2)
    t = tn.NativeTiles(gpu.default_params(2, voxel_size=0.1), tn.COMM_LOCAL, grp.handle, 0, 2, (2, 1), 5.0)
    try:
        assert _size_query(t, 0) == 0 and _size_query(t, 1) == 0
        for f in FRAMES:
            with pytest.raises(gpu.VgsError) as e:
                t.segment_boxes(f)
            assert e.value.status == gpu._lib.VGS_E_STATE
        for bad in (2, -1):
            with pytest.raises(gpu.VgsError) as e:
                t.segment_boxes(bad)
            assert e.value.status == gpu._lib.VGS_E_ARG
    finally:
        t.close()
        grp.close()


# ---------------------------------------------------------------- front end
def test_tiles_run_front_end_writes_the_table(gpu, tmp_path):
    parts, base = _layout(gpu, "2x2")
    for o in base:
        assert not isinstance(o, Exception), o
    b = base[0]["b"]["upright"]
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    prefix = str(tmp_path / "t")
    for r, p in enumerate(parts):
        np.ascontiguousarray(p, dtype=np.float32).tofile(f"{prefix}.{r}.f32")
    csv = str(tmp_path / "box.csv")
    out = subprocess.check_output([EXE, "--emulate", "2x2", "--pitch", repr(float(_pitch(N_PER))), "--voxel", "0.1", "--segment-boxes", csv,
                                   "--box-frame", "upright", prefix], text=True, timeout=300)
    kept = int(out.strip().splitlines()[-1].split()[1])
    tab = np.loadtxt(csv, delimiter=",", skiprows=1, ndmin=2)
    assert tab.shape == (kept, 22) and kept == b["lo3"].shape[0]
    assert np.array_equal(tab[:, 0], np.arange(kept))
    for name, sl in (("center3", slice(1, 4)), ("half3", slice(4, 7)), ("frame9", slice(7, 16)), ("lo3", slice(16, 19)), ("hi3", slice(19, 22))):
        assert np.array_equal(tab[:, sl], b[name]), name      # %.17g round-trips a double
