"""Absorbing the stranded and the small parts of a caller's per-POINT labelling on the device (vgs_absorb_point_label_parts,
csrc/labelabsorb.hip; Engine.absorb_label_parts) against tests/label_absorb_ref.py, the numpy restatement of the rule in include/vgs.h,
fed the engine's own point_voxel(), lists(0) and used flags.  Every comparison is `==`: the label array byte for byte and all eight
counts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import label_absorb_ref as R
from label_components_ref import label_components
from label_refine_ref import floor_and_wall
from label_refine_scenes import GROUP5, SPLIT, WALL, _voxel_points, big_boundary_voxel, blob, dropped_beside_kept, grid_supervoxels

pytestmark = pytest.mark.gpu

# GROUP5's nodes under the default cut: unused voxels are inert, the stored rows pruned to used neighbours (tests/test_gpu_label_graph.py)
PRUNED5 = dict(voxel_size=0.1, graph_size=0.25, points_min=5, voxels_min=2)
CORNER = np.array([[0.1, 0.1, 0.1]])   # the octree's first box (tests/segment_scenes.py); the point carries no label


def _vgs(gpu, xyz, **kw):
    eng = gpu.Engine(gpu.default_params(2, **kw))
    eng.set_points(xyz)
    eng.run()
    return eng


def _inputs(eng):
    return (eng.point_voxel(),) + tuple(eng.lists("adjacency")) + (eng.attributes()["used"].astype(bool),)


def _check(eng, inp, labels, K, **kw):
    """absorb_label_parts on the engine and by the restatement: equal labels and counts; returns the engine's result and the
    restatement's evaluations"""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    before = labels.copy()
    got = eng.absorb_label_parts(labels, K=K, **kw)
    trace = []
    ref = R.absorb(labels, inp[0], inp[1], inp[2], inp[3], K, trace=trace, **kw)
    print(kw, K, [got[k] for k in R.COUNTS], [ref[k] for k in R.COUNTS])
    assert R.diff(got, ref) == [], R.diff(got, ref)
    assert got["labels"].dtype == np.int32 and got["labels"].shape == labels.shape and (labels == before).all()
    assert np.array_equal(eng.absorbed_labels(), got["labels"])
    return got, trace


def _voxel_of(xyz, ijk, voxel=0.1):
    with np.errstate(invalid="ignore"):
        return np.all(np.floor(xyz / np.float32(voxel)) == np.asarray(ijk, dtype=np.float32), axis=1)


def _row_scene(node_labels, per=8, step=2, seed=41):
    """voxels (2 + step * i, 2, 2) with `per` points each, labelled by node_labels; under GROUP5 (graph_size 0.25) voxels two steps
    apart touch and voxels four steps apart do not, so step = 2 gives a chain in which only consecutive voxels touch"""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([CORNER] + [_voxel_points(rng, (2 + step * i, 2, 2), per) for i in range(len(node_labels))]).astype(np.float32)
    labels = np.concatenate([[-1], np.repeat(node_labels, per)]).astype(np.int32)
    return xyz, labels


# ---------------------------------------------------------------- the engine's own labels
_wall = {}


def _wall_scene(gpu):
    if not _wall:
        xyz, truth = floor_and_wall()
        eng = _vgs(gpu, xyz, **WALL)
        eng.refine_labels()
        _wall.update(xyz=xyz, truth=truth, eng=eng, inp=_inputs(eng), own=eng.point_labels(), refined=eng.refined_labels())
    return _wall


@pytest.mark.parametrize("which", ["own", "refined"])
def test_the_engines_own_labels(gpu, which):
    s = _wall_scene(gpu)
    eng, inp, labels, K = s["eng"], s["inp"], s[which], s["eng"].counts()["kept"]
    assert K >= 2
    sizes = np.sort(label_components(labels, inp[0], inp[1], inp[2], K)["part_points"])
    assert sizes[-1] > sizes[-2] > 0
    got, _ = _check(eng, inp, labels, K)   # the default parameters: the identity
    assert np.array_equal(got["labels"], labels) and got["rounds"] == 0 and got["candidates_left"] == 0
    _check(eng, inp, labels, K, min_points=0, island_points=50)
    _check(eng, inp, labels, K, min_points=3, island_points=0, drop=True)
    # every part but the largest is below the threshold, and floor and wall touch: something is absorbed
    got, _ = _check(eng, inp, labels, K, min_points=int(sizes[-2]) + 1, island_points=0)
    assert got["parts_absorbed"] > 0 and got["rounds"] >= 1 and got["points_relabelled"] > 0


def test_a_planted_island(gpu):
    s = _wall_scene(gpu)
    eng, inp, xyz, truth, own, K = s["eng"], s["inp"], s["xyz"], s["truth"], s["own"], s["eng"].counts()["kept"]
    floor_l = int(np.bincount(own[(truth == 0) & (own >= 0)]).argmax())
    wall_l = int(np.bincount(own[(truth == 1) & (own >= 0)]).argmax())
    assert floor_l != wall_l
    # an interior floor voxel, 2 m from the wall and from the floor's edges: its points take the wall's label
    mid = int(np.argmin(np.where(truth == 0, np.abs(xyz[:, 0] - 2.1) + np.abs(xyz[:, 1] - 2.1), np.inf)))
    isl = inp[0] == inp[0][mid]
    n_isl = int(isl.sum())
    assert n_isl > 1 and (truth[isl] == 0).all() and (own[isl] == floor_l).all()
    labels = own.copy()
    labels[isl] = wall_l
    got, _ = _check(eng, inp, labels, K, island_points=n_isl + 1)
    assert (got["labels"][isl] == floor_l).all() and got["parts_absorbed"] >= 1
    got, _ = _check(eng, inp, labels, K, island_points=n_isl)   # strictly below: a part of exactly the threshold stays
    assert (got["labels"][isl] == wall_l).all()


# ---------------------------------------------------------------- several labels per node
@pytest.mark.parametrize("mod,min_points", [(3, 100), (3, 400), (70, 3), (70, 10)])
def test_several_labels_per_node(gpu, mod, min_points):
    """(5 000, 300, 40 and 25 points in four voxels, one of them isolated: with three labels the vertices hold 1 667, 100, 13 and 8
    points, with seventy 71, 4 and 1)"""
    xyz = big_boundary_voxel()
    eng = _vgs(gpu, xyz, **SPLIT)
    inp = _inputs(eng)
    labels = np.arange(xyz.shape[0]) % mod
    _check(eng, inp, labels, mod, min_points=min_points)
    _check(eng, inp, labels, mod, min_points=min_points, island_points=4 * min_points, drop=True)
    # the isolated voxel (the last 25 points) with twenty points of label 0 and five of label 1: a stable part and a candidate whose only
    # link is the node they share
    labels = labels.copy()
    labels[-25:-5], labels[-5:] = 0, 1
    got, trace = _check(eng, inp, labels, mod, min_points=10)
    assert got["parts_absorbed"] >= 1 and (got["labels"][-5:] == 0).all() and (trace[0][3][trace[0][1]] >= 1).any()


def _many_labels_in_a_node():
    """Three voxels out of each other's reach.  Each holds n stable labels of 10 .. 22 points (five of them tie at 22) and ONE point of
    a label of its own: a candidate whose only links are the n shared nodes -- n = 66, 64 and 130 records, a wavefront has 64 lanes."""
    rng = np.random.default_rng(43)
    pts, lab = [CORNER], [[-1]]
    for ijk, first, n, lone in (((10, 10, 10), 0, 66, 500), ((40, 10, 10), 100, 64, 501), ((70, 10, 10), 300, 130, 502)):
        sizes = [10 + (j * 7) % 13 for j in range(n)]
        pts.append(_voxel_points(rng, ijk, sum(sizes) + 1))
        lab.append(np.concatenate([np.repeat(np.arange(first, first + n), sizes), [lone]]))
    order = rng.permutation(sum(p.shape[0] for p in pts) - 1) + 1   # the labels of a node in no particular point order
    xyz, labels = np.concatenate(pts).astype(np.float32), np.concatenate(lab).astype(np.int32)
    return np.concatenate([xyz[:1], xyz[order]]), np.concatenate([labels[:1], labels[order]]), 503


def test_more_records_than_lanes(gpu):
    xyz, labels, K = _many_labels_in_a_node()
    eng = _vgs(gpu, xyz, **SPLIT)
    inp = _inputs(eng)
    got, trace = _check(eng, inp, labels, K, min_points=5)
    cmp, cand, target, n_rec = trace[0]
    assert sorted(n_rec[cand].tolist()) == [64, 66, 130]   # exactly 64, above 64, above 128
    links = R.label_graph(cmp["part_of_point"], inp[0], inp[1], inp[2], inp[3], cmp["n_parts"])
    assert (links["n_pairs"] == 0).all() and (links["n_shared"] == 1).all()   # every link is a shared node only
    # most points, then the lower part id: the first label of 22 points of each voxel (j = 11)
    assert got["rounds"] == 1 and got["parts_absorbed"] == 3 and got["points_relabelled"] == 3
    for lone, first in ((500, 0), (501, 100), (502, 300)):
        assert got["labels"][labels == lone].tolist() == [first + 11]


# ---------------------------------------------------------------- rounds
@pytest.mark.parametrize("drop", [False, True], ids=["keep", "drop"])
@pytest.mark.parametrize("max_rounds", [0, 2, 3, 4])
def test_a_chain_of_three_rounds(gpu, max_rounds, drop):
    node_labels = [0] * 6 + [1, 2, 3]
    xyz, labels = _row_scene(node_labels)
    eng = _vgs(gpu, xyz, **GROUP5)
    got, _ = _check(eng, _inputs(eng), labels, 4, min_points=16, max_rounds=max_rounds, drop=drop)
    # each small voxel touches its predecessor only: one is absorbed per round
    done = min(max_rounds, 3)
    assert got["rounds"] == done and got["parts_absorbed"] == done and got["points_relabelled"] == 8 * done
    assert got["candidates_left"] == 3 - done and got["points_dropped"] == (8 * (3 - done) if drop else 0)
    want = [0] * (6 + done) + [(-1 if drop else l) for l in node_labels[6 + done:]]
    assert got["labels"][1:].reshape(-1, 8).tolist() == [[l] * 8 for l in want]


@pytest.mark.parametrize("node_labels,want", [([0, 0, 0, 1, 2, 2, 2], 0), ([0, 0, 1, 2, 2, 2, 2], 2)], ids=["by_id", "by_size"])
def test_tie_breaks(gpu, node_labels, want):
    xyz, labels = _row_scene(node_labels)
    eng = _vgs(gpu, xyz, **GROUP5)
    got, trace = _check(eng, _inputs(eng), labels, 3, min_points=16)
    assert trace[0][3][trace[0][1]].tolist() == [2]   # the one candidate has both neighbours as records, one contact each
    mid = node_labels.index(1)
    assert got["rounds"] == 1 and (got["labels"][1 + 8 * mid:9 + 8 * mid] == want).all()


# ---------------------------------------------------------------- unused endpoints
def test_unused_endpoints(gpu):
    xyz = dropped_beside_kept()
    kept = np.any([_voxel_of(xyz, (2 + i, 2, 2)) for i in range(4)], axis=0)
    bridge = _voxel_of(xyz, (2, 2, 3)) | _voxel_of(xyz, (2, 2, 4))
    top = np.any([_voxel_of(xyz, (2 + i, 2, 5)) for i in range(2)], axis=0)
    labels = np.full(xyz.shape[0], -1, np.int32)
    labels[kept], labels[bridge], labels[top] = 0, 1, 2
    out = []
    for params in (GROUP5, PRUNED5):
        eng = _vgs(gpu, xyz, **params)
        inp = _inputs(eng)
        assert not inp[3][np.unique(inp[0][bridge])].any()   # the bridge voxels are unused
        got, _ = _check(eng, inp, labels, 3, min_points=20)
        # five contacts with the kept row, four with the pair above: the bridge goes to the kept row
        assert got["rounds"] == 1 and got["parts_absorbed"] == 1 and got["points_relabelled"] == 8 and (got["labels"][bridge] == 0).all()
        out.append(got)
    assert R.diff(out[0], out[1]) == []


# ---------------------------------------------------------------- degenerate inputs
def test_degenerate_inputs(gpu):
    xyz = dropped_beside_kept()
    eng = _vgs(gpu, xyz, **GROUP5)
    inp = _inputs(eng)
    n = xyz.shape[0]
    finite = np.isfinite(xyz).all(axis=1)
    got, _ = _check(eng, inp, np.full(n, -1, np.int32), 0, min_points=9, drop=True)   # K = 0
    assert got["n_parts"] == 0 and got["rounds"] == 0
    got, _ = _check(eng, inp, np.full(n, -1, np.int32), 3, min_points=9, drop=True)   # all labels negative
    assert got["n_parts"] == 0 and (got["labels"] == -1).all()
    two = np.where(finite, np.arange(n) % 2, 1).astype(np.int32)
    got, _ = _check(eng, inp, two, 2, min_points=1000, max_rounds=0)   # the cap at once
    assert got["rounds"] == 0 and np.array_equal(got["labels"], two) and got["candidates_left"] == got["n_parts"] > 0
    got, _ = _check(eng, inp, two, 2)   # the default parameters: the identity
    assert got["rounds"] == 0 and np.array_equal(got["labels"], two) and got["n_skipped"] == 4
    # a labelled non-finite point keeps its label, also under drop
    got, _ = _check(eng, inp, two, 2, min_points=1000, drop=True)
    assert got["n_skipped"] == 4 and (got["labels"][~finite] == 1).all() and (got["labels"][finite] == -1).all()
    assert got["points_dropped"] == int(finite.sum())


@pytest.mark.parametrize("kind", ["no_finite_point", "empty_cloud"])
def test_clouds_without_a_node(gpu, kind):
    xyz = np.full((5, 3), np.nan, np.float32) if kind == "no_finite_point" else np.zeros((0, 3), np.float32)
    eng = _vgs(gpu, xyz, **GROUP5)
    n = xyz.shape[0]
    labels = (np.arange(n) % 2).astype(np.int32)
    got = eng.absorb_label_parts(labels, min_points=3, drop=True, K=2)
    assert np.array_equal(got["labels"], labels) and got["n_skipped"] == n and got["n_parts"] == 0 and got["rounds"] == 0


# ---------------------------------------------------------------- SVGS
def test_svgs_grid_supervoxels(gpu):
    xyz = blob(n=6000)
    sv, mx = grid_supervoxels(xyz)
    eng = gpu.Engine(gpu.default_params(3))
    eng.set_points(xyz)
    eng.set_supervoxel_labels(sv, mx)
    eng.svgs_segment()
    inp = _inputs(eng)
    labels = (xyz[:, 0] > 0).astype(np.int32) + (xyz[:, 1] > 0.4)
    _check(eng, inp, labels, 3, min_points=40, island_points=400)
    _check(eng, inp, np.maximum(sv - 1, -1), mx, min_points=30, drop=True)   # every supervoxel a label of its own
    _check(eng, inp, eng.point_labels(), eng.counts()["kept"], min_points=200, island_points=1000)


# ---------------------------------------------------------------- determinism and isolation
def test_determinism_and_isolation(gpu):
    torch = pytest.importorskip("torch")
    lib = gpu._lib
    xyz = np.random.default_rng(8).uniform(0.0, 1.2, size=(6_000, 3)).astype(np.float32)
    eng = _vgs(gpu, xyz, **GROUP5)
    eng.refine_labels()
    own, refined, K = eng.point_labels(), eng.refined_labels(), 9
    # stripes of 0.25 along x in three labels, every eleventh point one of six other labels: small parts strewn over the stripes
    labels = (np.floor(xyz[:, 0] / 0.25).astype(np.int32) % 3).astype(np.int32)
    labels[::11] = 3 + np.arange(labels[::11].shape[0]) % 6
    labels[::53] = -1
    kw = dict(min_points=20, island_points=200, drop=True)
    seg = eng.segment_graph()
    a, _ = _check(eng, _inputs(eng), labels, K, **kw)
    assert a["parts_absorbed"] > 0
    assert R.diff(eng.absorb_label_parts(labels, K=K, **kw), a) == []
    assert R.diff(_vgs(gpu, xyz, **GROUP5).absorb_label_parts(labels, K=K, **kw), a) == []
    dev = torch.from_numpy(labels).to("cuda:0")
    assert R.diff(eng.absorb_label_parts(dev, K=K, **kw), a) == [] and R.diff(eng.absorb_label_parts(dev, **kw), a) == []   # K None: max + 1
    assert np.array_equal(dev.cpu().numpy(), labels)   # read in place, never written
    # the device pointer hands out the same labelling
    back = np.zeros(labels.shape[0], np.int32)
    hip = C.cdll.LoadLibrary("libamdhip64.so")
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(eng.absorbed_labels_device_ptr()), C.c_size_t(back.nbytes), 2) == 0
    assert np.array_equal(back, a["labels"])
    # no other label buffer and no other table is touched
    assert np.array_equal(eng.point_labels(), own) and np.array_equal(eng.refined_labels(), refined)
    seg2 = eng.segment_graph()
    assert all(seg2[k].tobytes() == seg[k].tobytes() for k in seg)
    helpers.check_graph(eng)

    def fails(call):
        with pytest.raises(gpu.VgsError) as e:
            call()
        assert e.value.status == lib.VGS_E_STATE, e.value

    # the results of the two inner passes are overwritten: their getters refuse until their own next compute call
    eng.label_components(labels, K)
    eng.label_graph(labels, K)
    eng.label_components_device(), eng.label_graph_device()
    eng.absorb_label_parts(labels, K=K, **kw)
    fails(eng.label_components_device)
    fails(eng.label_graph_device)
    fails(lambda: eng._ck(eng._L.vgs_get_point_label_components(eng._h, *([None] * 7))))
    fails(lambda: eng._ck(eng._L.vgs_get_point_label_graph(eng._h, *([None] * 8))))
    eng.label_components(labels, K)
    eng.label_components_device()
    fails(eng.label_graph_device)
    eng.label_graph(labels, K)
    eng.label_graph_device()
    assert np.array_equal(eng.absorbed_labels(), a["labels"])   # and they leave the absorbed labels where they are


# ---------------------------------------------------------------- the status contract
def test_status_contract(gpu):
    lib = gpu._lib
    xyz = dropped_beside_kept()
    n = xyz.shape[0]
    labels = (np.arange(n) % 2).astype(np.int32)
    eng = gpu.Engine(gpu.default_params(2, **GROUP5))
    eng.set_points(xyz)
    ptr = labels.ctypes.data_as(C.c_void_p)

    def fails(call, status):
        with pytest.raises(gpu.VgsError) as e:
            call()
        assert e.value.status == status, e.value
        return str(e.value)

    def raw(p=ptr, n_=n, K=2, ap=(1, 0, 8, 0), null_params=False):
        a = lib.AbsorbParams(*ap)
        return lambda: eng._ck(eng._L.vgs_absorb_point_label_parts(eng._h, p, n_, K, None if null_params else C.byref(a), None))

    ap = lib.AbsorbParams(5, 6, 7, 1)
    assert eng._L.vgs_absorb_params_default(C.byref(ap)) == 0
    assert (ap.min_points, ap.island_points, ap.max_rounds, ap.drop) == (0, 0, 8, 0)
    fails(lambda: eng.absorb_label_parts(labels, K=2), lib.VGS_E_STATE)   # before a run
    eng.run()
    fails(eng.absorbed_labels, lib.VGS_E_STATE)   # the getters before a compute call
    fails(eng.absorbed_labels_device_ptr, lib.VGS_E_STATE)
    fails(lambda: eng.absorb_label_parts(labels[:-1], K=2), lib.VGS_E_ARG)   # n != N
    fails(raw(p=None), lib.VGS_E_ARG)   # NULL labels
    assert "params" in fails(raw(null_params=True), lib.VGS_E_ARG)
    fails(raw(K=-1), lib.VGS_E_ARG)
    fails(raw(K=1 << 31), lib.VGS_E_ARG)
    assert "min_points" in fails(raw(ap=(-1, 0, 8, 0)), lib.VGS_E_ARG)
    assert "island_points" in fails(raw(ap=(0, -1, 8, 0)), lib.VGS_E_ARG)
    assert "max_rounds" in fails(raw(ap=(1, 0, -1, 0)), lib.VGS_E_ARG)
    assert "max_rounds" in fails(raw(ap=(1, 0, 65, 0)), lib.VGS_E_ARG)
    raw(ap=(1, 0, 64, 0))()
    bad = labels.copy()
    bad[7], bad[11] = 3, 9
    assert "labels[7] = 3" in fails(lambda: eng.absorb_label_parts(bad, min_points=2, K=3), lib.VGS_E_ARG)   # the first offending index
    fails(eng.absorbed_labels, lib.VGS_E_STATE)   # ... and it left no result behind
    eng.absorb_label_parts(labels, min_points=2, K=2)
    eng.absorbed_labels(), eng.absorbed_labels_device_ptr()
    eng.run()   # a new run of the stages
    fails(eng.absorbed_labels, lib.VGS_E_STATE)
    # a tile context is refused, the limitation named
    t = gpu.Engine(gpu.default_params(2, **GROUP5))
    t.set_points(xyz)
    lo, hi = np.array([-1e9, -1e9], dtype=np.float64), np.array([1e9, 1e9], dtype=np.float64)
    t._ck(t._L.vgs_set_owned_region(t._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    t.run()
    msg = fails(lambda: t.absorb_label_parts(labels, min_points=2, K=2), lib.VGS_E_STATE)
    assert "tile context" in msg and "across the ranks" in msg and "does not exist yet" in msg
    assert "does not exist yet" in fails(t.absorbed_labels, lib.VGS_E_STATE)


# ---------------------------------------------------------------- the front end
def test_front_end_absorbs_a_class_field(gpu, tmp_path):
    """vgs_run --absorbed-labels over --class-field / --classes: the written .i32 equals Engine.absorb_label_parts on the same input"""
    from test_cpp_segment_desc import CSRC, RUN, VGS_LINES, _write_task
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    xyz = gpu.scenes.town_scene(30_000)
    cell = np.floor(xyz[:, :2].astype(np.float64)).astype(np.int64)
    cls = ((cell[:, 0] + 2 * cell[:, 1]) % 6 - 1).astype(np.int32)   # classes -1 .. 4 in 1 m cells of the ground plan
    cls[::997] = 4                                                   # and a few single points of class 4 strewn over the others
    gpu.pcd.write_pcd(tmp_path / "in.pcd", xyz, mode="binary", extra={"cls": cls})
    lines = dict(VGS_LINES)
    lines.update({12: str(tmp_path) + "/", 15: "in.pcd", 18: str(tmp_path) + "/", 21: "out.pcd"})
    task, path = str(tmp_path / "task.txt"), str(tmp_path / "a.i32")
    _write_task(task, 2, lines)
    out = subprocess.run([RUN, task, "--absorbed-labels", path, "--class-field", "cls", "--classes", "5", "--absorb-islands", "3"],
                         check=True, capture_output=True, text=True).stdout
    eng = _vgs(gpu, xyz)
    want = eng.absorb_label_parts(cls, island_points=3, K=5)   # (parts of one or two points that are not their class's largest)
    assert want["parts_absorbed"] > 0
    assert np.fromfile(path, dtype=np.int32).tobytes() == want["labels"].tobytes()
    line = [l for l in out.splitlines() if l.startswith("absorbed ")]
    assert len(line) == 1 and [int(v) for v in line[0].split()[1:]] == [want[k] for k in gpu.Engine.ABSORB_COUNTS]
    assert os.path.getsize(path) == 4 * xyz.shape[0]
