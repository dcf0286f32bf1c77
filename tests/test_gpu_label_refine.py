"""Point-level label refinement on the device (vgs_refine_point_labels, csrc/refine.hip) against tests/label_refine_ref.py, the numpy
float32 restatement of the rule in include/vgs.h, over the engine's own outputs -- compared with `==`, no tolerance:
  * VGS on the floor-and-wall scene and on a 20 k-point blob, SVGS through set_supervoxel_labels; near the origin and shifted by FAR;
  * one test at each structural limit of the kernels: a boundary voxel of 5 000 points (several batches, batches starting inside a node),
    rows longer than one candidate chunk, a labelled node whose only candidate is itself, unlabelled nodes without a candidate, a dropped
    cluster beside a kept one, a mirror-symmetric pair of nodes with a point on the symmetry plane (equal costs: the smaller id wins),
    NaN points, patch_radius 0 and 10^6;
  * the interface: identical bytes from call to call, other parameters on the same context, no side effect on point_labels() and
    helpers.snapshot, the status codes, the counts.
(tests/segment_scenes.py has no blob; the one here is test_gpu_segment_graph.py's: 20 000 points, N(0, 0.3).)"""
import ctypes as C

import numpy as np
import pytest

import helpers
from label_refine_ref import floor_and_wall, node_state, refine_cost, refine_labels, working_nodes
from label_refine_scenes import (FAR, GROUP5, SPLIT, SPLIT5, WALL, big_boundary_voxel, blob, dropped_beside_kept, grid_supervoxels,
                                 mirror_pair)

pytestmark = pytest.mark.gpu

RF_BATCH = 256   # points per work item (csrc/refine.hip)
RF_CH = 256      # candidates staged per chunk


def _vgs(gpu, xyz, **kw):
    eng = gpu.Engine(gpu.default_params(2, **kw))
    eng.set_points(xyz)
    eng.run()
    return eng


def _svgs(gpu, xyz, labels, max_label, **kw):
    eng = gpu.Engine(gpu.default_params(3, **kw))
    eng.set_points(xyz)
    eng.set_supervoxel_labels(labels, max_label)
    eng.svgs_segment()
    return eng


def _inputs(eng, xyz):
    return dict(xyz=xyz, point_voxel=eng.point_voxel(), attr=eng.attributes(), kept=eng.node_labels()[1], adjacency=eng.lists("adjacency"))


def _ref(inp, patch_radius, switch_ratio=0.25, fill=True):
    return refine_labels(inp["xyz"], inp["point_voxel"], inp["attr"], inp["kept"], inp["adjacency"], patch_radius, switch_ratio, fill)


def _default_radius(eng):
    return eng.params.seed_size if eng.params.method == 3 else eng.params.voxel_size


def _check(eng, inp, patch_radius=None, switch_ratio=0.25, fill=True):
    """refine on the engine and by the restatement: equal labels, equal counts; returns (labels, counts)"""
    counts = eng.refine_labels(patch_radius, switch_ratio, fill)
    got = eng.refined_labels()
    ref, rc = _ref(inp, _default_radius(eng) if patch_radius is None else patch_radius, switch_ratio, fill)
    print(counts)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], ref[bad[:8]], inp["point_voxel"][bad[:8]])
    assert counts == rc
    return got, counts


def _far(xyz):
    return (xyz.astype(np.float64) + np.asarray(FAR)).astype(np.float32)


def _wall_svgs(gpu, shift):
    xyz = floor_and_wall()[0][::4]
    labels, mx = grid_supervoxels(xyz)
    if shift:
        xyz = _far(xyz)
    return xyz, _svgs(gpu, xyz, labels, mx)


SCENES = {
    "wall": lambda gpu: (lambda xyz: (xyz, _vgs(gpu, xyz, **WALL)))(floor_and_wall()[0]),
    "wall_far": lambda gpu: (lambda xyz: (xyz, _vgs(gpu, xyz, **WALL)))(_far(floor_and_wall()[0])),
    "blob": lambda gpu: (lambda xyz: (xyz, _vgs(gpu, xyz)))(blob()),
    "blob_far": lambda gpu: (lambda xyz: (xyz, _vgs(gpu, xyz)))(_far(blob())),
    "blob_split": lambda gpu: (lambda xyz: (xyz, _vgs(gpu, xyz, **dict(SPLIT, points_min=3))))(blob()),
    "svgs_wall": lambda gpu: _wall_svgs(gpu, False),
    "svgs_wall_far": lambda gpu: _wall_svgs(gpu, True),
}
_cache = {}


def _scene(gpu, name):
    """(inputs of the restatement, segmented engine) of a scene, made once and shared; the tests leave the segmentation unchanged"""
    if name not in _cache:
        xyz, eng = SCENES[name](gpu)
        _cache[name] = (_inputs(eng, xyz), eng)
    return _cache[name]


# ---------------------------------------------------------------- the engine against the restatement
@pytest.mark.parametrize("name", sorted(SCENES))
def test_equals_restatement(gpu, name):
    inp, eng = _scene(gpu, name)
    got, counts = _check(eng, inp)
    assert counts["working_nodes"] > 0 and counts["points_examined"] > 0
    if name == "wall":
        # the cases this scene stands for: labelled boundary nodes, interior nodes, a dropped cluster beside a kept one, unused voxels
        A, _ = node_state(inp["attr"], inp["kept"])
        work = working_nodes(inp["attr"], inp["kept"], inp["adjacency"])
        used = inp["attr"]["used"] != 0
        assert (work & (A >= 0)).any() and (~work & (A >= 0)).any() and (work & used & (A < 0)).any() and (work & ~used).any()
        assert counts["points_changed"] > 0 and counts["points_filled"] > 0 and (got >= 0).all()


# ---------------------------------------------------------------- structural limits
def test_boundary_voxel_of_5000_points(gpu):
    xyz = big_boundary_voxel()
    eng = _vgs(gpu, xyz, **SPLIT5)
    inp = _inputs(eng, xyz)
    npts = np.bincount(inp["point_voxel"], minlength=eng.counts()["voxels"])
    big = int(np.argmax(npts))
    work = working_nodes(inp["attr"], inp["kept"], inp["adjacency"])
    assert npts[big] == 5000 and npts[big] > 2 * RF_BATCH and npts[big] % RF_BATCH != 0 and work[big]
    got, counts = _check(eng, inp)
    assert counts["points_examined"] >= 5000 and counts["points_changed"] > 0
    # a labelled node whose only candidate is itself: interior, its points keep their label
    off, idx = inp["adjacency"]
    alone = [v for v in range(len(npts)) if inp["attr"]["used"][v] and set(idx[off[v]:off[v + 1]]) <= {v}]
    assert alone and not work[alone].any()
    m = np.isin(inp["point_voxel"], alone)
    assert (got[m] == inp["kept"][inp["point_voxel"][m]]).all() and (got[m] >= 0).all()


def test_rows_longer_than_one_candidate_chunk(gpu):
    xyz = blob(5, 20_000, 0.15)
    eng = _vgs(gpu, xyz, voxel_size=0.05, graph_size=0.5, cut_thred=0.0, points_min=3, voxels_min=0, adjacency_min=1_000_000)
    inp = _inputs(eng, xyz)
    off, idx = inp["adjacency"]
    used = inp["attr"]["used"] != 0
    assert max(int(used[idx[off[v]:off[v + 1]]].sum()) for v in np.flatnonzero(used)) > 2 * RF_CH   # used neighbours: what a stored row holds
    _check(eng, inp)


def test_nodes_without_candidates_dropped_cluster_and_nan_points(gpu):
    xyz = dropped_beside_kept()
    eng = _vgs(gpu, xyz, **GROUP5)
    inp = _inputs(eng, xyz)
    A, cand = node_state(inp["attr"], inp["kept"])
    work = working_nodes(inp["attr"], inp["kept"], inp["adjacency"])
    used = inp["attr"]["used"] != 0
    assert eng.counts()["kept"] == 1
    assert (used & (A < 0) & ~work).any()     # the dropped cluster: its rows hold unlabelled nodes only
    assert (~used & work).any()               # unused voxels that reach the kept cluster
    assert (~used & ~work).any()              # an unused voxel that reaches nothing
    got, counts = _check(eng, inp)
    pv = inp["point_voxel"]
    assert (got[pv < 0] == -1).all() and (pv[-4:] < 0).all()                      # NaN and infinite points
    assert (got[(pv >= 0) & ~work[np.maximum(pv, 0)] & (A[np.maximum(pv, 0)] < 0)] == -1).all()
    assert counts["points_filled"] == int(((pv >= 0) & work[np.maximum(pv, 0)]).sum()) > 0
    g0, c0 = _check(eng, inp, fill=False)
    assert c0 == dict(working_nodes=0, points_examined=0, points_changed=0, points_filled=0)
    assert np.array_equal(g0, eng.point_labels())


def test_equal_costs_the_smaller_node_id_wins(gpu):
    xyz, labels, mx = mirror_pair()
    eng = _svgs(gpu, xyz, labels, mx, cut_thred=0.0, adjacency_min=1_000_000)
    inp = _inputs(eng, xyz)
    pv, kept = inp["point_voxel"], inp["kept"]
    a, b, c = int(pv[0]), int(pv[60]), int(pv[-1])
    assert len({a, b, c}) == 3 and len({int(kept[a]), int(kept[b]), int(kept[c])}) == 3 and kept.min() >= 0
    cost = refine_cost(xyz[-1:], inp["attr"]["centroid"][[a, b, c]], inp["attr"]["normal"][[a, b, c]], 0.25)[0]
    assert cost[0].view(np.uint32) == cost[1].view(np.uint32) and cost[0] < np.float32(0.25) * cost[2]
    got, _ = _check(eng, inp, patch_radius=0.25)
    assert got[-1] == kept[min(a, b)] != kept[max(a, b)]


def test_patch_radius_zero_and_huge(gpu):
    inp, eng = _scene(gpu, "wall")
    g0, _ = _check(eng, inp, patch_radius=0.0)
    g1, _ = _check(eng, inp, patch_radius=1.0e6)
    assert not np.array_equal(g0, g1)


# ---------------------------------------------------------------- interface
def test_calls_repeat_and_other_parameters(gpu):
    inp, eng = _scene(gpu, "wall")
    a, ca = _check(eng, inp)
    b, cb = _check(eng, inp)
    assert a.tobytes() == b.tobytes() and ca == cb
    pl = eng.point_labels()
    s0, c0 = _check(eng, inp, switch_ratio=0.0)
    assert (s0[pl >= 0] == pl[pl >= 0]).all() and c0["points_changed"] == 0
    s1, _ = _check(eng, inp, switch_ratio=1.0, patch_radius=0.1)
    assert not np.array_equal(s1, a)
    n0, cn = _check(eng, inp, fill=False)
    assert (n0[pl < 0] == -1).all() and cn["points_filled"] == 0
    # the device pointer holds what the host getter copies
    assert eng.refined_labels_device_ptr()
    eng.refine_labels()
    hip = C.CDLL("libamdhip64.so")
    h = np.zeros(eng.n, dtype=np.int32)
    assert hip.hipMemcpy(h.ctypes.data_as(C.c_void_p), C.c_void_p(eng.refined_labels_device_ptr()), C.c_size_t(h.nbytes), 2) == 0   # DeviceToHost
    assert np.array_equal(h, a)


def test_no_side_effects(gpu):
    inp, eng = _scene(gpu, "blob")
    before = helpers.snapshot(eng)
    pl = eng.point_labels()
    _check(eng, inp)
    assert np.array_equal(eng.point_labels(), pl)
    helpers.assert_same_snapshot(before, helpers.snapshot(eng))
    _check(eng, inp)   # the getters of the snapshot (the full adjacency pass among them) leave the refinement's inputs as they were


def test_status_codes(gpu):
    lib = gpu._lib
    xyz = blob()
    eng = gpu.Engine(gpu.default_params(2))
    with pytest.raises(gpu.VgsError) as e:
        eng.refine_labels()
    assert e.value.status == lib.VGS_E_STATE
    eng.set_points(xyz)
    eng.voxelize(); eng.features(); eng.adjacency()
    with pytest.raises(gpu.VgsError) as e:
        eng.refine_labels()
    assert e.value.status == lib.VGS_E_STATE
    eng.segment()
    for getter in (eng.refined_labels, eng.refined_labels_device_ptr):   # segmented, no refine yet
        with pytest.raises(gpu.VgsError) as e:
            getter()
        assert e.value.status == lib.VGS_E_STATE
    for kw in (dict(patch_radius=-0.1), dict(patch_radius=float("nan")), dict(patch_radius=float("inf")), dict(switch_ratio=-0.01),
               dict(switch_ratio=1.01), dict(switch_ratio=float("nan"))):
        with pytest.raises(gpu.VgsError) as e:
            eng.refine_labels(**kw)
        assert e.value.status == lib.VGS_E_ARG, kw
    with pytest.raises(gpu.VgsError) as e:   # a refused refine leaves none behind
        eng.refined_labels()
    assert e.value.status == lib.VGS_E_STATE
    eng.refine_labels(patch_radius=0.0, switch_ratio=1.0)
    a = eng.refined_labels()
    assert a.shape == (xyz.shape[0],)
    eng.run()   # a new run drops the refinement
    with pytest.raises(gpu.VgsError) as e:
        eng.refined_labels()
    assert e.value.status == lib.VGS_E_STATE
    # a tile context is refused
    t = gpu.Engine(gpu.default_params(2))
    t.set_points(xyz)
    lo, hi = np.array([-1e9, -1e9], dtype=np.float64), np.array([1e9, 1e9], dtype=np.float64)
    t._ck(t._L.vgs_set_owned_region(t._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    t.run()
    with pytest.raises(gpu.VgsError) as e:
        t.refine_labels()
    assert e.value.status == lib.VGS_E_STATE
    # no point at all: nothing to refine, nothing to read
    z = gpu.Engine(gpu.default_params(2))
    z.set_points(np.zeros((0, 3), dtype=np.float32))
    z.run()
    assert z.refine_labels() == dict(working_nodes=0, points_examined=0, points_changed=0, points_filled=0)
    assert z.refined_labels().shape == (0,)


def test_class_mirror(gpu):
    xyz = floor_and_wall()[0]
    s = gpu.VoxelBasedSegmentation(0.25)
    s.setInputCloud(xyz); s.getCloudPointNum(xyz); s.addPointsFromInputCloud()
    s.setVoxelSize(0.25, 10, 3, 3)
    s.setVoxelCenters(); s.calcualteVoxelCloudAttributes(xyz); s.findAllVoxelAdjacency(0.6)
    s.segmentVoxelCloudWithGraphModel(0.3, 0.2, 0.2, 0.2, 0.2, 0.2, 2.0)
    assert (s.refineClusterLabels() == -1).all()
    s.drawColorMapofPointsinClusters()
    r = s.refineClusterLabels()
    inp = _inputs(s.engine, xyz)
    assert np.array_equal(r, _check(s.engine, inp)[0]) and (r >= 0).all()
    assert np.array_equal(s.refineClusterLabels(patch_radius=0.1, switch_ratio=0.5, fill=False), _check(s.engine, inp, 0.1, 0.5, False)[0])
    xyz2, labels, mx = mirror_pair()
    v = gpu.SuperVoxelBasedSegmentation(0.05)
    v.setInputCloud(xyz2); v.addPointsFromInputCloud()
    with pytest.raises(gpu.VgsError) as err:
        v.refineClusterLabels()
    assert err.value.status == gpu._lib.VGS_E_STATE
