"""Point-level label refinement across the ranks of the native tiled driver (vgs_tiles_refine_point_labels, include/vgs_tiles.h), ranks as
threads of this process over LocalGroup on one GPU.  Every point is evaluated by the rank that loaded it; the concatenation of the ranks'
refined labels must equal, with ==, what tests/label_refine_ref.py -- the numpy restatement of the rule in include/vgs.h -- gives on the
gathered points with the tiled global labels.

The oracle does not depend on how the tiled and the single engine number or cut their segments: a plain Engine on np.concatenate(parts)
(rank order is the order a tile assembles, so the node records match) supplies point_voxel, attributes and adjacency; every voxel takes
the tiled global label of its points (all points of a voxel must agree); the restatement runs with those labels.
  * scenes: the floor-and-wall scene of label_refine_ref split by y at 2.06 (the seam crosses the tile border), scenes.tiled_urban_scene
    in the 2x1 and 2x2 layouts and 2x2 far from the origin; fill on and off everywhere, switch_ratio 0 and 1 and patch_radius 0 on the
    wall; preconditions from the plain engine's outputs, so that no case passes vacuously; a voxel of 5 000 points on the tile border,
    so that each rank's share of one node spans several batches;
  * protocol: one all_gather_varlen per call, header + 16 bytes per band record on the first call and the header alone afterwards, the
    same bytes from call to call and from run to run, no side effect on labels, descriptors, graph and boxes in either order;
  * one rank equals a plain engine byte for byte; failures; points handed to the wrong rank; the front end."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import label_refine_ref as LR
from label_refine_scenes import SPLIT5, WALL, big_boundary_voxel
from test_gpu_tiles_segdesc import _parts, _pitch, _ranks, _same
from test_gpu_tiles_segfields import LAYOUTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")
N_PER = 60_000          # points per rank of the urban layouts: the restatement is a Python loop over the voxels
HEADER = 32             # bytes of the refine payload's header: two 16-byte entries
WALL_BORDER = 2.06      # the tile border of the wall scene, in y
BIG_BORDER = 0.25       # the tile border through the voxel of 5 000 points (y in [0.2, 0.3]) of big_boundary_voxel
RF_BATCH = 256          # points per work item (csrc/refine.hip)
# (patch_radius, switch_ratio, fill); None = the context's default
PARAMS = {"default": (None, None, True), "nofill": (None, None, False), "sr0": (None, 0.0, True), "sr1": (None, 1.0, True), "pr0": (0.0, None, True)}
SCENES = {"wall": tuple(PARAMS), "2x1": ("default", "nofill"), "2x2": ("default", "nofill"), "2x2_far": ("default", "nofill")}
_cache = {}


# ---------------------------------------------------------------- scenes and their geometry
def _scene_def(gpu, name):
    """(parts, tiles, pitch, center, engine params as kwargs)"""
    if name == "wall":
        xyz = LR.floor_and_wall(seed=1, n=20_000)[0]
        low = xyz[:, 1].astype(np.float64) < WALL_BORDER
        return [xyz[low], xyz[~low]], (1, 2), 4.0, (0.0, WALL_BORDER), dict(WALL)   # rank 0's points first: the chained grid's order
    tiles, shift = LAYOUTS[name]
    return _parts(gpu, tiles, N_PER, shift), tiles, _pitch(N_PER), (tuple(shift[:2]) if shift else (0.0, 0.0)), dict(voxel_size=0.1)


def _owner(xy, tiles, pitch, center):
    """rank that owns a voxel centre: tile (i, j) of the layout, the outer tiles open ended (vgs_tiles_create)"""
    tx, ty = tiles
    i = np.clip(np.floor((xy[:, 0].astype(np.float64) - (center[0] - tx / 2.0 * pitch)) / pitch), 0, tx - 1).astype(np.int64)
    j = np.clip(np.floor((xy[:, 1].astype(np.float64) - (center[1] - ty / 2.0 * pitch)) / pitch), 0, ty - 1).astype(np.int64)
    return j * tx + i


def _plain(gpu, xyz, kw):
    eng = gpu.Engine(gpu.default_params(2, **kw))
    eng.set_points(xyz)
    eng.run()
    return eng


def _voxel_labels(pv, labels, V, skip=None):
    """the tiled global label of every voxel from its points' labels; all points of a voxel (but the skipped ones) must agree"""
    m = pv >= 0
    if skip is not None:
        m &= ~skip
    lo = np.full(V, np.iinfo(np.int32).max, np.int64)
    hi = np.full(V, -2, np.int64)
    np.minimum.at(lo, pv[m], labels[m])
    np.maximum.at(hi, pv[m], labels[m])
    assert (hi >= -1).all(), "a voxel without a point to take its label from"
    assert np.array_equal(lo, hi), f"{int((lo != hi).sum())} voxels hold points of two labels"
    return lo.astype(np.int32)


def _inputs(gpu, parts, kw, labels, skip=None):
    """the restatement's inputs from a plain engine on the gathered points, with the tiled labels"""
    xyz = np.concatenate(parts)
    eng = _plain(gpu, xyz, kw)
    pv = eng.point_voxel()
    attr = eng.attributes()
    inp = dict(xyz=xyz, point_voxel=pv, attr=attr, adjacency=eng.lists("adjacency"), centers=eng.voxel_centers(),
               kept=_voxel_labels(pv, labels, attr["used"].shape[0], skip), voxel_size=kw["voxel_size"])
    return inp


def _ref(inp, which):
    pr, sr, fill = PARAMS[which]
    return LR.refine_labels(inp["xyz"], inp["point_voxel"], inp["attr"], inp["kept"], inp["adjacency"], inp["voxel_size"] if pr is None else pr,
                            0.25 if sr is None else sr, fill)


def _best_candidate(inp, pts, patch_radius):
    """node id of the rule's best candidate -- smallest (cost, id) -- for the points pts (-1: none)"""
    off, idx = inp["adjacency"]
    _, cand = LR.node_state(inp["attr"], inp["kept"])
    cen = np.ascontiguousarray(inp["attr"]["centroid"], dtype=np.float32)
    nrm = np.ascontiguousarray(inp["attr"]["normal"], dtype=np.float32)
    out = np.full(pts.size, -1, np.int64)
    pv = inp["point_voxel"][pts]
    for v in np.unique(pv):
        sel = np.flatnonzero(pv == v)
        w = LR.candidates_of(int(v), off, idx, cand)
        if w.size == 0:
            continue
        cost = LR.refine_cost(np.ascontiguousarray(inp["xyz"][pts[sel]], dtype=np.float32)[:, :3], cen[w], nrm[w], patch_radius)
        cost = np.where(np.isfinite(cost), cost, np.float32(np.inf))
        b = np.argmin(cost, axis=1)
        ok = np.isfinite(cost[np.arange(sel.size), b])
        out[sel[ok]] = w[b[ok]]
    return out


def preconditions(inp, rank_of, owner, ref, name):
    """what makes a scene cover the new ground, from the plain engine's outputs and the restatement's result at the default parameters:
    points loaded by a rank that does not own their voxel, some in working nodes; a refined point that takes the label of a candidate
    another rank owns; a filled point of an unused voxel whose best candidate another rank owns"""
    pv = inp["point_voxel"]
    A, _ = LR.node_state(inp["attr"], inp["kept"])
    inside = pv >= 0
    before = np.where(inside, A[np.maximum(pv, 0)], -1)
    work = LR.working_nodes(inp["attr"], inp["kept"], inp["adjacency"], True)
    foreign = inside & (owner[np.maximum(pv, 0)] != rank_of)
    assert foreign.sum() > 0 and work[pv[foreign]].any(), (name, int(foreign.sum()))
    moved = np.flatnonzero(inside & (ref != before) & (ref >= 0))
    best = _best_candidate(inp, moved, inp["voxel_size"])
    assert (best >= 0).all() and np.array_equal(inp["kept"][best], ref[moved])
    across = owner[best] != rank_of[moved]
    assert across.any(), (name, "no refined point takes the label of a candidate of another rank")
    unused = inp["attr"]["used"][pv[moved]] == 0
    assert (across & unused & (before[moved] < 0)).any(), (name, "no filled point of an unused voxel has its best candidate on another rank")
    return dict(foreign=int(foreign.sum()), across=int(across.sum()), across_fill=int((across & unused).sum()))


# ---------------------------------------------------------------- one tiled run per scene, shared
def _collect(r, t, xyz, which):
    t.set_points(xyz)
    t.run()
    labels, kept = t.point_labels()
    res, pay, times = {}, {}, {}
    for w in which:
        counts = t.refine_labels(*PARAMS[w])
        res[w] = (t.refined_labels().copy(), counts)
        pay[w] = t.refine_payload()
        times[w] = t.refine_times()
    counts2 = t.refine_labels(*PARAMS[which[0]])                      # the first parameters again: the same bytes, the header alone
    second = np.array_equal(t.refined_labels(), res[which[0]][0]) and counts2 == res[which[0]][1]
    pay_second = t.refine_payload()
    labels_after, _ = t.point_labels()
    t.run()
    try:
        t.refined_labels()
        stale = None
    except Exception as ex:  # noqa: BLE001
        stale = ex
    counts3 = t.refine_labels(*PARAMS[which[0]])                      # a new run: the band travels again, the same bytes
    rerun = np.array_equal(t.refined_labels(), res[which[0]][0]) and counts3 == res[which[0]][1]
    return dict(labels=labels, kept=kept, res=res, pay=pay, times=times, second=second, pay_second=pay_second, rerun=rerun,
                pay_rerun=t.refine_payload(), stale=stale, labels_equal=bool(np.array_equal(labels, labels_after)))


def _scene(gpu, name):
    """(scene definition, per-rank results, the restatement's inputs) of a scene, made once and shared"""
    if name not in _cache:
        parts, tiles, pitch, center, kw = _scene_def(gpu, name)
        out = _ranks(gpu, tiles, pitch, parts, lambda r, t, p: _collect(r, t, p, SCENES[name]), center=center, params=gpu.default_params(2, **kw))
        for r, o in enumerate(out):
            assert not isinstance(o, Exception), (name, r, o)
        inp = _inputs(gpu, parts, kw, np.concatenate([o["labels"] for o in out]))
        _cache[name] = ((parts, tiles, pitch, center, kw), out, inp, {})
    return _cache[name]


def _restated(gpu, name, which):
    _, _, inp, refs = _scene(gpu, name)
    if which not in refs:
        refs[which] = _ref(inp, which)
    return refs[which]


# ---------------------------------------------------------------- the ranks against the restatement
@pytest.mark.parametrize("name,which", [(n, w) for n in SCENES for w in SCENES[n]])
def test_equals_restatement(gpu, name, which):
    (parts, tiles, pitch, center, kw), out, inp, _ = _scene(gpu, name)
    ref, rc = _restated(gpu, name, which)
    got = np.concatenate([o["res"][which][0] for o in out])
    counts = [o["res"][which][1] for o in out]
    print(name, which, counts, rc)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], ref[bad[:8]], inp["point_voxel"][bad[:8]])
    for key in ("working_nodes", "points_examined", "points_changed", "points_filled"):
        assert sum(c[key] for c in counts) == rc[key], (key, counts, rc)
    assert all(c["points_beyond_strip"] == 0 for c in counts)
    if which == "sr0":
        assert rc["points_changed"] == 0 and rc["points_filled"] > 0      # no labelled point changes
    if which == "nofill":
        assert rc["points_filled"] == 0
    if name == "wall" and which == "default":
        assert all(c["points_changed"] > 0 for c in counts), counts        # the seam crosses the border: both ranks change labels


@pytest.mark.parametrize("name", list(SCENES))
def test_the_scenes_cover_the_new_ground(gpu, name):
    (parts, tiles, pitch, center, kw), out, inp, _ = _scene(gpu, name)
    rank_of = np.repeat(np.arange(len(parts)), [p.shape[0] for p in parts])
    owner = _owner(inp["centers"], tiles, pitch, center)
    print(name, preconditions(inp, rank_of, owner, _restated(gpu, name, "default")[0], name))


def test_a_border_voxel_of_5000_points_split_between_two_ranks(gpu):
    """label_refine_scenes.big_boundary_voxel laid out as the wall scene is, the tile border at y = 0.25 through the voxel of 5 000 points:
    each rank's share of it spans several batches, the last one partial, and in every batch only some lanes hold a point of the rank's own
    load.  (The other scenes give no voxel more than RF_BATCH points.)"""
    kw = dict(SPLIT5)
    xyz = big_boundary_voxel()
    low = xyz[:, 1].astype(np.float64) < BIG_BORDER
    parts = [xyz[low], xyz[~low]]                                     # rank 0's points first: the chained grid's order
    which = ("default", "nofill")

    def body(r, t, p):
        t.set_points(p)
        t.run()
        labels, _ = t.point_labels()
        return labels, {w: (t.refine_labels(*PARAMS[w]), t.refined_labels().copy()) for w in which}
    out = _ranks(gpu, (1, 2), 4.0, parts, body, center=(0.0, BIG_BORDER), params=gpu.default_params(2, **kw))
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    inp = _inputs(gpu, parts, kw, np.concatenate([o[0] for o in out]))
    # from the plain engine's outputs: the voxel holds 5 000 points, is a working node, and each rank loaded more than a batch of them
    pv = inp["point_voxel"]
    npts = np.bincount(pv[pv >= 0], minlength=inp["attr"]["used"].shape[0])
    big = int(np.argmax(npts))
    assert npts[big] == 5000 and npts[big] > 2 * RF_BATCH and npts[big] % RF_BATCH != 0
    assert LR.working_nodes(inp["attr"], inp["kept"], inp["adjacency"], False)[big]
    rank_of = np.repeat(np.arange(2), [p.shape[0] for p in parts])
    share = np.bincount(rank_of[pv == big], minlength=2)
    print(share)
    assert (share > RF_BATCH).all(), share
    for w in which:
        ref, rc = _ref(inp, w)
        got = np.concatenate([o[1][w][1] for o in out])
        counts = [o[1][w][0] for o in out]
        print(w, counts, rc)
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (w, bad.size, bad[:8], got[bad[:8]], ref[bad[:8]], pv[bad[:8]])
        for key in ("working_nodes", "points_examined", "points_changed", "points_filled"):
            assert sum(c[key] for c in counts) == rc[key], (w, key, counts, rc)
        assert all(c["points_beyond_strip"] == 0 for c in counts), (w, counts)


@pytest.mark.parametrize("name", list(SCENES))
def test_payload_repeats_and_reruns(gpu, name):
    """the first call of a run carries the band, later calls the header alone; a second call and a second run give the same bytes"""
    _, out, _, _ = _scene(gpu, name)
    first = SCENES[name][0]
    for r, o in enumerate(out):
        n_band = o["pay"][first]["band_records"]
        assert n_band > 0 and o["pay"][first]["bytes_sent"] == HEADER + 16 * n_band, (r, o["pay"][first])
        for w in SCENES[name][1:]:
            assert o["pay"][w] == dict(band_records=0, bytes_sent=HEADER), (r, w, o["pay"][w])
        assert o["pay_second"] == dict(band_records=0, bytes_sent=HEADER)
        assert o["pay_rerun"] == o["pay"][first]                            # compacted in voxel order: the same payload
        assert o["second"] and o["rerun"] and o["labels_equal"]
        assert isinstance(o["stale"], gpu.VgsError) and o["stale"].status == gpu._lib.VGS_E_STATE, o["stale"]
        t = o["times"][first]
        assert t["total"] > 0 and t["refine"] > 0 and min(t.values()) >= 0


# ---------------------------------------------------------------- side effects, in both orders of graph and refine
def _tables(t):
    labels, kept = t.point_labels()
    d = dict(labels=labels, kept=np.array([kept]))
    for k, v in t.segment_descriptors().items():
        d["d_" + k] = v
    for k, v in t.segment_graph().items():
        d["g_" + k] = v
    for f in ("principal", "upright"):
        for k, v in t.segment_boxes(f).items():
            d[f"b_{f}_{k}"] = v
    return d


def test_no_side_effect_on_labels_descriptors_graph_and_boxes(gpu):
    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        a = _tables(t)                                     # graph first ...
        t.refine_labels()
        fine = t.refined_labels().copy()
        b = _tables(t)                                     # (cached tables)
        own = t.own_segment_graph(a["kept"][0])            # ... and computed again from the graph's own halo table, after the refine
        t.run()
        t.refine_labels()                                  # refine first ...
        fine2 = t.refined_labels().copy()
        c = _tables(t)                                     # ... then descriptors, graph and boxes, computed behind it
        t.refine_labels()
        return _same(a, b), _same(a, c), bool(np.array_equal(fine, fine2) and np.array_equal(fine, t.refined_labels())), own
    parts = _parts(gpu, (2, 1), N_PER)
    out = _ranks(gpu, (2, 1), _pitch(N_PER), parts, body)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
        assert o[0] and o[1] and o[2], (r, o[:3])
        assert o[3]["seg_ab"].shape[0] > 0


# ---------------------------------------------------------------- one rank
def test_one_rank_equals_a_plain_engine_with_one_exchange_per_call(gpu):
    """1x1 through a communicator that counts: the labels and counts are a plain engine's, byte for byte, and a call makes two all-gathers
    -- the sizes and the padded payload of ONE all_gather_varlen -- and no broadcast"""
    from vgs_svgs_segmentation_amd import tiles_native as tn
    xyz = _parts(gpu, (1, 1), N_PER)[0]
    calls = dict(ag=0, bc=0)

    def ag(send, recv):
        calls["ag"] += 1
        recv[:] = send

    def bc(buf, root):
        calls["bc"] += 1
    t = tn.NativeTiles.with_callbacks(gpu.default_params(2, voxel_size=0.1), 0, 1, (1, 1), _pitch(N_PER), ag, bc)
    try:
        t.set_points(xyz)
        t.run()
        eng = _plain(gpu, xyz, dict(voxel_size=0.1))
        assert np.array_equal(eng.point_labels(), t.point_labels()[0])
        for w, (pr, sr, fill) in PARAMS.items():
            before = dict(calls)
            counts = t.refine_labels(pr, sr, fill)
            assert (calls["ag"] - before["ag"], calls["bc"] - before["bc"]) == (2, 0), (w, before, calls)
            want = eng.refine_labels(pr, 0.25 if sr is None else sr, fill)
            assert counts.pop("points_beyond_strip") == 0 and counts == want, (w, counts, want)
            assert np.array_equal(t.refined_labels(), eng.refined_labels()), w
            assert t.refine_payload() == dict(band_records=0, bytes_sent=HEADER)     # one region: no border line within reach
    finally:
        t.close()


class _Meet:
    """the host transport of `world` rank threads through the driver's callbacks, counting every rank's calls"""

    def __init__(self, world):
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.calls = [dict(ag=0, bc=0) for _ in range(world)]

    def callbacks(self, r):
        def ag(send, recv):
            self.calls[r]["ag"] += 1
            self.slots[r] = np.array(send, copy=True)
            self.barrier.wait(60)
            recv[:] = np.concatenate(self.slots)
            self.barrier.wait(60)

        def bc(buf, root):
            self.calls[r]["bc"] += 1
            if r == root:
                self.slots[root] = np.array(buf, copy=True)
            self.barrier.wait(60)
            if r != root:
                buf[:] = self.slots[root]
            self.barrier.wait(60)
        return ag, bc


def test_two_ranks_make_one_exchange_per_call_with_and_without_the_band(gpu):
    """2x1 through a communicator that counts: the call that carries the band records and the calls that carry the header alone each make
    two all-gathers -- the sizes and the padded payload of ONE all_gather_varlen -- and no broadcast, on both ranks"""
    from vgs_svgs_segmentation_amd import tiles_native as tn
    parts = _parts(gpu, (2, 1), N_PER)
    meet = _Meet(2)
    out = [None, None]

    def rank_main(r):
        try:
            ag, bc = meet.callbacks(r)
            t = tn.NativeTiles.with_callbacks(gpu.default_params(2, voxel_size=0.1), r, 2, (2, 1), _pitch(N_PER), ag, bc)
            try:
                t.set_points(parts[r])
                t.run()
                rows = []
                for fill in (True, False, True):
                    before = dict(meet.calls[r])
                    t.refine_labels(fill=fill)
                    rows.append((meet.calls[r]["ag"] - before["ag"], meet.calls[r]["bc"] - before["bc"], t.refine_payload()["band_records"]))
                out[r] = rows
            finally:
                t.close()
        except Exception as ex:  # noqa: BLE001
            out[r] = ex
            meet.barrier.abort()
    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(300.0)
    assert not any(t.is_alive() for t in th)
    for r, rows in enumerate(out):
        assert not isinstance(rows, Exception), (r, rows)
        assert [x[:2] for x in rows] == [(2, 0)] * 3, (r, rows)
        assert rows[0][2] > 0 and rows[1][2] == rows[2][2] == 0, (r, rows)


# ---------------------------------------------------------------- failures
def _status(gpu, x):
    assert isinstance(x, gpu.VgsError), x
    return x.status


def _run_then(gpu, call, timeout=120.0):
    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        return call(r, t, xyz)
    return _ranks(gpu, (2, 1), _pitch(N_PER), _parts(gpu, (2, 1), N_PER), body, timeout=timeout)


def test_a_failing_rank_takes_its_peer_out(gpu, monkeypatch):
    monkeypatch.setenv("VGS_TILES_FAIL_RANK", "1")
    monkeypatch.setenv("VGS_TILES_FAIL_AT", "refine")
    out = _run_then(gpu, lambda r, t, xyz: t.refine_labels())
    assert _status(gpu, out[1]) == gpu._lib.VGS_E_STATE and "refine" in str(out[1]), out[1]
    assert _status(gpu, out[0]) == gpu._lib.VGS_E_PEER and "rank 1" in str(out[0]), out[0]


def test_ranks_that_disagree_on_a_parameter_all_return_arg(gpu):
    def call(r, t, xyz):
        try:
            t.refine_labels(switch_ratio=0.25 if r == 0 else 0.5)
        except gpu.VgsError as ex:
            first = ex
        else:
            first = None
        return first, t.refine_labels(), t.refined_labels()           # the handle is still good, and the band has travelled
    out = _run_then(gpu, call)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
        assert _status(gpu, o[0]) == gpu._lib.VGS_E_ARG and "rank 1" in str(o[0]) and "rank 0" in str(o[0]), o[0]
        assert o[1]["points_examined"] > 0 and o[2].shape[0] > 0


def test_a_nan_patch_radius_travels_in_the_status_word(gpu):
    out = _run_then(gpu, lambda r, t, xyz: t.refine_labels(patch_radius=float("nan") if r == 1 else None))
    assert _status(gpu, out[1]) == gpu._lib.VGS_E_ARG and "patch_radius" in str(out[1]), out[1]
    assert _status(gpu, out[0]) == gpu._lib.VGS_E_PEER and "rank 1" in str(out[0]), out[0]


def test_bad_calls_are_refused_without_a_collective(gpu):
    """one rank of two, whose peer never calls: the errors come back, so they are decided locally"""
    from vgs_svgs_segmentation_amd import tiles_native as tn
    grp = tn.LocalGroup(2)
    t = tn.NativeTiles(gpu.default_params(2, voxel_size=0.1), tn.COMM_LOCAL, grp.handle, 0, 2, (2, 1), 5.0)
    try:
        with pytest.raises(gpu.VgsError) as e:
            t.refine_labels()
        assert e.value.status == gpu._lib.VGS_E_STATE and "vgs_tiles_run first" in str(e.value)
        with pytest.raises(gpu.VgsError) as e:
            t.refined_labels()
        assert e.value.status == gpu._lib.VGS_E_STATE
    finally:
        t.close()
        grp.close()


def test_context_calls_keep_their_sides(gpu):
    """vgs_refine_point_labels still refuses a tile context, vgs_refine_own_point_labels and its two companions refuse a plain one, and
    refined_labels() needs a refine since the last run"""
    L = gpu._lib.lib()
    E = gpu._lib.VGS_E_STATE

    def call(r, t, xyz):
        h = t._ctx()
        rp = gpu._lib.VgsRefineParams()
        assert L.vgs_refine_params_default(h, C.byref(rp)) == 0
        st = [t._L.vgs_tiles_get_refined_labels(t._h, np.zeros(xyz.shape[0] + 1, np.int32).ctypes.data_as(C.c_void_p))]   # a run, no refine yet
        st.append(L.vgs_refine_point_labels(h, C.byref(rp), None))
        msg = L.vgs_last_error_string(h)
        t.refine_labels()
        st.append(t._L.vgs_tiles_get_refined_labels(t._h, np.zeros(xyz.shape[0] + 1, np.int32).ctypes.data_as(C.c_void_p)))
        # the stages run again on the context, with no new labels of the tile and no new halo labels: the table of the last run is gone
        seg = (L.vgs_segment(h), L.vgs_refine_own_point_labels(h, C.byref(rp), None), L.vgs_last_error_string(h))
        t.set_points(xyz)
        st.append(t._L.vgs_tiles_get_refined_labels(t._h, np.zeros(xyz.shape[0] + 1, np.int32).ctypes.data_as(C.c_void_p)))   # new points: gone
        return st, msg, seg
    for o in _run_then(gpu, call):
        assert not isinstance(o, Exception), o
        assert o[0] == [E, E, 0, E] and b"tile context" in o[1], o
        assert o[2][0] == 0 and o[2][1] == E and b"vgs_set_refine_halo_labels" in o[2][2], o[2]
    eng = _plain(gpu, _parts(gpu, (1, 1), N_PER)[0][:20_000], dict(voxel_size=0.1))
    rp = gpu._lib.VgsRefineParams()
    assert L.vgs_refine_params_default(eng._h, C.byref(rp)) == 0
    n = C.c_int64(0)
    assert L.vgs_refine_own_point_labels(eng._h, C.byref(rp), None) == E and b"tile context" in L.vgs_last_error_string(eng._h)
    assert L.vgs_get_own_band_labels(eng._h, C.byref(n), None, None) == E
    assert L.vgs_set_refine_halo_labels(eng._h, None, None, 0) == E


# ---------------------------------------------------------------- points handed to the wrong rank
def test_points_loaded_beyond_the_strip_keep_their_label(gpu):
    """five points from deep inside rank 1's region are handed to rank 0: the call succeeds, rank 0 reports them in points_beyond_strip and
    leaves them their point label; every other point still equals the restatement"""
    parts = _parts(gpu, (2, 1), N_PER)
    pitch = _pitch(N_PER)
    deep = np.flatnonzero((parts[1][:, 0] > 0.4 * pitch) & (parts[1][:, 0] < 0.6 * pitch))[:5]
    assert deep.size == 5
    moved = [np.concatenate([parts[0], parts[1][deep]]), np.delete(parts[1], deep, axis=0)]

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        labels, _ = t.point_labels()
        counts = t.refine_labels()
        return labels, counts, t.refined_labels().copy(), t.info()
    out = _ranks(gpu, (2, 1), pitch, moved, body)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    # (the urban tiles themselves reach a few decimetres over their edges: those points are refined like any other)
    outside = [[int((_owner(p[:, :2], (2, 1), pitch, (0.0, 0.0)) != r).sum()) for r, p in enumerate(ps)] for ps in (parts, moved)]
    assert [o[3]["n_outside"] for o in out] == outside[1] == [outside[0][0] + 5, outside[0][1]], (outside, out[0][3], out[1][3])
    assert out[0][1]["points_beyond_strip"] == 5 and out[1][1]["points_beyond_strip"] == 0
    n0 = moved[0].shape[0]
    assert np.array_equal(out[0][2][n0 - 5:], out[0][0][n0 - 5:])                       # they keep their point_labels() value
    labels = np.concatenate([out[0][0], out[1][0]])
    skip = np.zeros(labels.shape[0], bool)
    skip[n0 - 5:n0] = True
    inp = _inputs(gpu, moved, dict(voxel_size=0.1), labels, skip=skip)
    ref, rc = _ref(inp, "default")
    got = np.concatenate([out[0][2], out[1][2]])
    assert np.array_equal(got[~skip], ref[~skip]), int((got[~skip] != ref[~skip]).sum())
    assert rc["points_changed"] > 0 and rc["points_filled"] > 0


# ---------------------------------------------------------------- front end
def test_tiles_run_front_end_writes_the_refined_labels(gpu, tmp_path):
    (parts, tiles, pitch, center, kw), out, _, _ = _scene(gpu, "2x1")
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    prefix = str(tmp_path / "t")
    for r, p in enumerate(parts):
        np.ascontiguousarray(p, dtype=np.float32).tofile(f"{prefix}.{r}.f32")
    for flags, which in (([], "default"), (["--no-fill"], "nofill")):
        txt = subprocess.check_output([EXE, "--emulate", "2x1", "--pitch", repr(float(pitch)), "--voxel", "0.1", "--refine"] + flags + [prefix],
                                      text=True, timeout=300)
        lines = txt.strip().splitlines()
        assert int(lines[0].split()[1]) == out[0]["kept"] and lines[1].split()[0] == "refine"
        counts = [o["res"][which][1] for o in out]
        want = [sum(c[k] for c in counts) for k in ("working_nodes", "points_examined", "points_changed", "points_filled", "points_beyond_strip")]
        assert [int(x) for x in lines[1].split()[1:]] == want, (lines[1], want)
        for r, o in enumerate(out):
            assert np.array_equal(np.fromfile(f"{prefix}.{r}.refined.i32", dtype=np.int32), o["res"][which][0]), (which, r)
            assert np.array_equal(np.fromfile(f"{prefix}.{r}.labels.i32", dtype=np.int32), o["labels"]), (which, r)
