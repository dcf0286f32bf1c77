"""One context over a sequence of DIFFERING clouds (include/vgs.h: vgs_set_points / vgs_stage_points / vgs_commit_points,
vgs_get_point_labels_async / vgs_wait_point_labels, vgs_host_alloc; INTEGRATION.md's loop).

A reused context carries grow-only buffers, two input buffers that flip, two label buffers that swap under a download, and a dozen cached
tables and flags keyed on parameters or on "the last run".  A fresh engine has zeroed counters, unset flags and exactly sized buffers --
the state that hides a stale read -- so every test here runs frames of different size, content, voxel-key layout and emptiness
(tests/sequence_frames.py) through ONE engine and demands that every result of frame k equals, byte for byte, what a fresh Engine gives
on the same cloud and parameters (helpers.snapshot), and that the labels equal the CPU oracle's.  There are no tolerances.

What these tests cannot prove: a copy stream that is not ordered behind its event can pass them by luck.  Neighbouring frames differ in
size and content, so a copy out of the wrong buffer or of the wrong cloud fails, but the ORDER of a copy and a kernel that happen to
finish in the right sequence is not observable from the host without a profiler."""
import ctypes as C

import numpy as np
import pytest

import sequence_frames as sf
from helpers import assert_same_snapshot, oracle_params, snapshot

pytestmark = pytest.mark.gpu

SENTINEL = -7777
EMPTY_FRAMES = ("F", "Z", "X")   # no used voxel, no point, no finite point: every schedule counter is 0, as on a fresh engine


def _params(gpu, name):
    return gpu.default_params(2, **sf.PARAMS[name])


def _run_fresh(gpu, name):
    eng = gpu.Engine(_params(gpu, name))
    eng.set_points(sf.cloud(name))
    eng.run()
    return eng


class _Fresh:
    """Snapshots and labels of a fresh Engine per frame, computed once and shared (read-only) by the tests of this module."""

    def __init__(self, gpu):
        self.gpu, self._snap = gpu, {}

    def snap(self, name):
        if name not in self._snap:
            s = snapshot(_run_fresh(self.gpu, name))
            for a in s.values():
                a.setflags(write=False)
            self._snap[name] = s
        return self._snap[name]

    def labels(self, name):
        return self.snap(name)["point_labels"]


@pytest.fixture(scope="module")
def fresh(gpu):
    return _Fresh(gpu)


@pytest.fixture(scope="module")
def refs(oracle, gpu):
    return {k: oracle.run_vgs(sf.cloud(k), oracle_params(oracle, _params(gpu, k))) for k in sf.ORACLE_FRAMES}


def _count(snap, key):
    return int(snap["counts"][list(snap["counts.names"]).index(key)])


def _check_frame(name, snap, refs):
    """What a snapshot of frame `name` must show whoever made it: the frame reached its case, and the oracle agrees."""
    n, v, depth, layout, used, kept = sf.EXPECT[name]
    assert _count(snap, "points") == n
    if layout is not None:
        assert sf.key_layout(_count(snap, "depth"), n) == layout, (name, _count(snap, "depth"))
    for key, want in (("voxels", v), ("used", used), ("kept", kept)):
        if want is not None:
            assert _count(snap, key) == want, (name, key)
    if name in EMPTY_FRAMES:
        assert not snap["schedule_counters"].any(), (name, dict(zip(snap["schedule_counters.names"], snap["schedule_counters"])))
        assert (snap["point_labels"] == -1).all()
        assert name == "F" or (snap["point_voxel"] == -1).all()
    if name in refs:
        np.testing.assert_array_equal(snap["point_labels"], refs[name].labels()[0])
        assert _count(snap, "kept") == refs[name].kept_clusters


def test_fresh_engines_agree_with_the_oracle_and_each_other(gpu, fresh, refs):
    """The yardstick itself: a fresh engine's snapshot of every frame shows the frame's case and the oracle's labels, and a second
    fresh engine on frame A gives the same bytes (a schedule counter that did not would be timing-dependent and is named in
    helpers.SNAPSHOT_TIMING_COUNTERS)."""
    for name in sf.EXPECT:
        _check_frame(name, fresh.snap(name), refs)
    assert_same_snapshot(snapshot(_run_fresh(gpu, "A")), fresh.snap("A"), "second fresh engine on A")


def test_reused_context_plain_set_points(gpu, fresh, refs):
    """Big then small; used, then no used voxel, no point, no voxel; the three key widths through the same code / perm buffers; A three
    times with the same bytes each time."""
    order = "AEHFAZDXCTA"
    eng = gpu.Engine(_params(gpu, order[0]))
    current = sf.PARAMS[order[0]]
    for i, name in enumerate(order):
        if sf.PARAMS[name] != current:   # in front of C and F, and back
            eng.set_params(_params(gpu, name))
            current = sf.PARAMS[name]
        eng.set_points(sf.cloud(name))
        eng.run()
        snap = snapshot(eng)
        assert_same_snapshot(snap, fresh.snap(name), f"frame {name} (position {i} of {order})")
        _check_frame(name, snap, refs)


def _buffers(gpu, pinned, shape, dtype, count):
    return [gpu.pinned_empty(shape, dtype) if pinned else np.empty(shape, dtype) for _ in range(count)]


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_staged_loop(gpu, fresh, pinned):
    """INTEGRATION.md's loop: the upload of cloud k+1 beside the stages of cloud k, the download of cloud k's labels beside the stages of
    cloud k+1; two alternating input buffers holding (N, 3) and (N, 4) rows in turn, two alternating label buffers.  Every downloaded
    array is the fresh engine's for ITS frame; frame k+1 differs from frame k in N or (C then A, 20000 points both) in most of its
    labels (test_sequence_frames_cpu.py), so a copy out of the wrong buffer cannot pass."""
    order = "AHEFZCA"
    n_max = max(sf.cloud(k).shape[0] for k in order)
    inbuf = _buffers(gpu, pinned, (n_max * 4,), np.float32, 2)
    outbuf = _buffers(gpu, pinned, (n_max + 64,), np.int32, 2)

    def fill(i):   # the host side of cloud i: rows of 12 and 16 bytes in turn
        xyz = sf.cloud(order[i]) if i % 2 == 0 else sf.padded(sf.cloud(order[i]))
        view = inbuf[i & 1][:xyz.size].reshape(xyz.shape)
        view[...] = xyz
        return view

    def check(i):   # download i is complete: its frame's labels, and nothing behind them
        n = sf.cloud(order[i]).shape[0]
        np.testing.assert_array_equal(outbuf[i & 1][:n], fresh.labels(order[i]), err_msg=f"labels of frame {order[i]} (position {i})")
        assert (outbuf[i & 1][n:] == SENTINEL).all(), (order[i], i)

    eng = gpu.Engine(_params(gpu, order[0]))
    eng.stage_points(fill(0))
    for i, name in enumerate(order):
        eng.commit_points()
        eng.set_params(_params(gpu, name))
        if i + 1 < len(order):
            eng.stage_points(fill(i + 1))          # the next cloud uploads beside this cloud's stages
        eng.run()
        assert eng.counts()["points"] == sf.cloud(name).shape[0]
        outbuf[i & 1][:] = SENTINEL                # (its last download, of frame i - 2, was checked one turn ago)
        eng.point_labels_async(outbuf[i & 1])      # waits for download i - 1, then starts this one beside the next cloud's stages
        if i > 0:
            check(i - 1)
    eng.wait_labels()
    check(len(order) - 1)
    assert_same_snapshot(snapshot(eng), fresh.snap(order[-1]), "the context after the staged loop")


def _raises_state(gpu, fn):
    with pytest.raises(gpu.VgsError) as e:
        fn()
    assert e.value.status == gpu._lib.VGS_E_STATE, str(e.value)


def test_staging_touches_nothing_current(gpu, fresh):
    eng = _run_fresh(gpu, "A")
    eng.stage_points(sf.cloud("H"))
    assert_same_snapshot(snapshot(eng), fresh.snap("A"), "A with H staged")
    eng.stage_points(sf.cloud("G"))                # replaces the staged cloud without a commit
    assert_same_snapshot(snapshot(eng), fresh.snap("A"), "A with G staged over H")
    eng.commit_points()
    # committed, not yet run: the results of the previous frame are gone, not handed out under the new cloud's name
    for getter in (eng.point_labels, eng.segment_descriptors, eng.clusters):
        _raises_state(gpu, getter)
    eng.run()
    assert_same_snapshot(snapshot(eng), fresh.snap("G"), "G committed over a replaced H")
    _raises_state(gpu, eng.commit_points)          # nothing staged
    assert_same_snapshot(snapshot(eng), fresh.snap("G"), "G after a refused commit")
    # set_points while a cloud is staged: both get their own result
    eng.stage_points(sf.cloud("H"))
    eng.set_points(sf.cloud("A"))
    eng.run()
    assert_same_snapshot(snapshot(eng), fresh.snap("A"), "A set while H is staged")
    eng.commit_points()
    eng.run()
    assert_same_snapshot(snapshot(eng), fresh.snap("H"), "H committed behind a set_points")
    # an empty staged cloud
    eng.stage_points(sf.cloud("Z"))
    eng.commit_points()
    eng.run()
    assert_same_snapshot(snapshot(eng), fresh.snap("Z"), "Z staged and committed")
    _raises_state(gpu, eng.commit_points)


def test_download_in_flight_survives_the_next_run(gpu, fresh):
    """The next run writes the OTHER label buffer (merge.hip swaps pt_label / pt_label_alt): with more points than the cloud under
    download, the buffer must be swapped, not grown under the copy."""
    n_h, n_a, n_g = (sf.cloud(k).shape[0] for k in "HAG")
    eng = gpu.Engine(_params(gpu, "H"))
    eng.wait_labels()                              # nothing open: a no-op
    eng.set_points(sf.cloud("H"))
    eng.run()
    out = gpu.pinned_empty((n_a + 64,), np.int32)
    out[:] = SENTINEL
    eng.point_labels_async(out)
    eng.set_points(sf.cloud("A"))                  # straight away: more points
    eng.run()
    eng.wait_labels()
    np.testing.assert_array_equal(out[:n_h], fresh.labels("H"))
    assert (out[n_h:] == SENTINEL).all()
    np.testing.assert_array_equal(eng.point_labels(), fresh.labels("A"))
    # once more with the buffers in each other's place: the small one is now the spare and must grow for G, away from the copy
    out[:] = SENTINEL
    eng.point_labels_async(out)
    eng.set_points(sf.cloud("G"))
    eng.run()
    eng.wait_labels()
    np.testing.assert_array_equal(out[:n_a], fresh.labels("A"))
    assert (out[n_a:] == SENTINEL).all()
    assert_same_snapshot(snapshot(eng), fresh.snap("G"), "G behind two downloads in flight")
    # two downloads with no wait between them both complete
    out2 = gpu.pinned_empty((n_g + 3,), np.int32)
    out[:] = SENTINEL
    out2[:] = SENTINEL
    eng.point_labels_async(out)
    eng.point_labels_async(out2)
    eng.wait_labels()
    for o in (out, out2):
        np.testing.assert_array_equal(o[:n_g], fresh.labels("G"))
        assert (o[n_g:] == SENTINEL).all()
    eng.wait_labels()
    # no point: nothing to copy, nothing left open
    eng.set_points(sf.cloud("Z"))
    eng.run()
    out[:] = SENTINEL
    eng.point_labels_async(out)
    eng.wait_labels()
    assert (out == SENTINEL).all()
    # no finite point: a download of 100 labels -1 out of a buffer that held G's
    eng.set_points(sf.cloud("X"))
    eng.run()
    eng.point_labels_async(out)
    eng.wait_labels()
    assert (out[:100] == -1).all() and (out[100:] == SENTINEL).all()


def _from_device(ptr, count, dtype):
    h = np.zeros(count, dtype=dtype)
    if count:
        hip = C.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(h.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(h.nbytes), 2) == 0   # DeviceToHost
    return h


def test_device_resident_results_follow_the_frame(gpu, fresh):
    eng = gpu.Engine(_params(gpu, "A"))
    current = sf.PARAMS["A"]
    for name in "AHFA":
        if sf.PARAMS[name] != current:
            eng.set_params(_params(gpu, name))
            current = sf.PARAMS[name]
        eng.set_points(sf.cloud(name))
        eng.run()
        want = fresh.snap(name)
        n, kept = sf.cloud(name).shape[0], sf.EXPECT[name][5]
        lab = _from_device(eng.point_labels_device_ptr(), n, np.int32)
        np.testing.assert_array_equal(lab, eng.point_labels())
        np.testing.assert_array_equal(lab, want["point_labels"])
        p_off, p_idx = eng.clusters_device()
        off = _from_device(p_off, kept + 1, np.int64)
        h_off, h_idx = eng.clusters()
        np.testing.assert_array_equal(off, h_off)
        np.testing.assert_array_equal(off, want["clusters.voxel_id.offsets"])
        idx = _from_device(p_idx, int(off[-1]), np.int32)
        np.testing.assert_array_equal(idx, h_idx)
        np.testing.assert_array_equal(idx, want["clusters.voxel_id.ids"])
        if name == "F":
            assert off.tolist() == [0]
        else:
            assert off[-1] == (lab >= 0).sum() > 0


def _unused_are_inert(p):
    """csrc/adjacency.hip, vgs_unused_are_inert, restated in float32: an edge to an unused voxel carries the weight of five distances of
    100; the unused voxels are inert -- and pruned from the stored adjacency rows -- unless that weight beats a singleton's threshold."""
    f = np.float32
    s, a, t, c, e = (f(100) * (f(1) / f(sig)) for sig in (p.sig_p, p.sig_n, p.sig_o, p.sig_c, p.sig_e))
    d = np.sqrt((((s * s + a * a) + t * t) + c * c) + e * e, dtype=f)
    with np.errstate(under="ignore"):
        w = np.exp((f(-0.5) * d) * (f(1) / (f(p.sig_w) * f(p.sig_w))), dtype=f)
    return not (w > f(1) - f(p.cut_thred) / f(1))


def _rows_hold_unused(eng):
    """Which branch the engine took, read from its results: vgs_get_local_weights reports a node's STORED row -- the used neighbours only
    when unused voxels are inert, every neighbour otherwise -- while vgs_get_lists(adjacency) always holds every neighbour."""
    used = eng.attributes()["used"].astype(bool)
    off, idx = eng.lists("adjacency")
    has_unused = np.add.reduceat((~used[idx]).astype(np.int64), off[:-1]) > 0
    v = int(np.nonzero(used & has_unused)[0][0])   # a used voxel with an unused neighbour inside graph_size
    ids, _ = eng.local_weights(v)
    assert set(ids.tolist()) <= set(idx[off[v]:off[v + 1]].tolist())
    return bool((~used[ids]).any())


def test_parameter_round_trip_on_one_cloud(gpu):
    """adj_tab_* (ball tables keyed on graph / voxel size), lc_ctab_* (screening table keyed on sigmas / cut), adj_pruned and the re-run
    of the adjacency stage inside vgs_segment when only the cut changes what the rows must hold."""
    xyz = sf.cloud("A")
    p1 = gpu.default_params(2)
    p2 = gpu.default_params(2, graph_size=0.45, voxel_size=0.1)
    p3 = gpu.default_params(2, cut_thred=1.2)      # 1 - cut < 0 <= any weight: unused voxels can merge, the rows must hold them
    assert _unused_are_inert(p1) and _unused_are_inert(p2) and not _unused_are_inert(p3)

    def fresh_snap(p):
        e = gpu.Engine(p)
        e.set_points(xyz)
        e.run()
        assert _rows_hold_unused(e) == (not _unused_are_inert(p))
        return snapshot(e)

    want = {k: fresh_snap(p) for k, p in (("p1", p1), ("p2", p2), ("p3", p3))}
    assert want["p1"]["point_labels"].tobytes() != want["p2"]["point_labels"].tobytes() != want["p3"]["point_labels"].tobytes()
    eng = gpu.Engine(p1)
    eng.set_points(xyz)
    eng.run()
    first = snapshot(eng)
    assert_same_snapshot(first, want["p1"], "P1")
    for key, p in (("p2", p2), ("p3", p3)):
        eng.set_params(p)
        eng.run()
        assert _rows_hold_unused(eng) == (not _unused_are_inert(p))
        assert_same_snapshot(snapshot(eng), want[key], key)
    # only the cut changes: the context keeps its adjacency stage, and vgs_segment alone must notice that the rows no longer fit
    eng.set_params(p1)
    eng.segment()
    assert not _rows_hold_unused(eng)
    assert_same_snapshot(snapshot(eng), want["p1"], "P1 by vgs_segment alone behind P3")
    eng.set_params(p3)
    eng.segment()
    assert _rows_hold_unused(eng)
    assert_same_snapshot(snapshot(eng), want["p3"], "P3 by vgs_segment alone behind P1")
    eng.set_params(p1)
    eng.run()
    last = snapshot(eng)
    assert_same_snapshot(last, want["p1"], "P1 again")
    assert_same_snapshot(last, first, "the last run against the first")


def _svgs_results(eng):
    sv, mx = eng.supervoxel_labels()
    out = dict(supervoxel_labels=sv, max_label=np.array([mx]), point_labels=eng.point_labels())
    out.update({"voxel_table." + k: v for k, v in eng.voxel_table().items()})
    out.update({"attributes." + k: v for k, v in eng.attributes().items()})
    c = eng.counts()
    out["counts"] = np.array([c[k] for k in ("points", "finite", "voxels", "used", "adj", "clusters", "kept", "supervoxels")], dtype=np.int64)
    return out


def test_svgs_over_a_sequence(gpu):
    """Method 3: the engine's own supervoxels on two clouds, a caller's labelling on a third, the first cloud again, then no point at all:
    the labelling's reset per cloud, the external flag and the restore of the context's own lattice in vccs.hip."""
    from test_gpu_svgs import grid_supervoxels
    p = gpu.default_params(3)
    third = sf.svgs_cloud("town")
    labels, max_label = grid_supervoxels(third, 0.25)

    def own(eng, xyz):
        eng.set_points(xyz)
        eng.run()

    def given(eng, xyz):
        eng.set_points(xyz)
        eng.set_supervoxel_labels(labels, max_label)
        eng.svgs_segment()

    steps = [("urban", own, sf.svgs_cloud("urban")), ("pc", own, sf.svgs_cloud("pc")), ("town, caller's labels", given, third),
             ("urban again", own, sf.svgs_cloud("urban")), ("no point", own, sf.cloud("Z"))]
    eng = gpu.Engine(p)
    got = []
    for what, drive, xyz in steps:
        drive(eng, xyz)
        got.append(_svgs_results(eng))
        fresh_eng = gpu.Engine(p)
        drive(fresh_eng, xyz)
        assert_same_snapshot(got[-1], _svgs_results(fresh_eng), what)
    assert got[0]["counts"][6] >= 2 and got[1]["counts"][6] >= 2      # kept segments (test_sequence_frames_cpu: 74 and 2)
    np.testing.assert_array_equal(got[2]["supervoxel_labels"], labels)
    assert_same_snapshot(got[3], got[0], "the fourth frame against the first")
