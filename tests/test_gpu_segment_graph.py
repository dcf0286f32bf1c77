"""Segment adjacency graph (vgs_get_segment_graph, csrc/seggraph.hip) against a numpy ground truth built from independent getters: the
neighbour rows (vgs_get_lists(0), checked against the oracle's adjacency lists or a brute-force radius search), the kept node labels
(Engine.node_labels) and the local cut's weights (Engine.local_weights, a separate kernel over the same vm_pair_weight).  VGS and SVGS
(PCL order, the synchronous variant, a caller's labelling), a ~2 M-point scene, a constructed scene of separate objects on a ground plane,
consistency with the descriptors' boxes, determinism, the call-state contract and the absence of side effects."""
import ctypes as C

import numpy as np
import pytest

from helpers import check_graph, oracle_params, ragged_sets

pytestmark = pytest.mark.gpu

FIELDS = ("seg_ab", "n_pairs", "n_finite", "nodes_ab", "w_sum", "w_min", "w_max")


def check_boxes(eng, got):
    """Every edge's two segment boxes lie within graph_size plus one voxel diagonal of each other."""
    p = eng.params
    box = eng.segment_descriptors()["bbox6"].astype(np.float64)
    A, B = box[got["seg_ab"][:, 0]], box[got["seg_ab"][:, 1]]
    gap = np.maximum(0.0, np.maximum(B[:, :3] - A[:, 3:], A[:, :3] - B[:, 3:]))
    lim = p.graph_size + (np.sqrt(3.0) * p.voxel_size if p.method == 2 else 0.0)
    assert (np.linalg.norm(gap, axis=1) <= lim * (1 + 1e-6)).all()


def _vgs(gpu, xyz, **kw):
    eng = gpu.Engine(gpu.default_params(2, **kw))
    eng.set_points(xyz)
    eng.run()
    return eng


# ---------------------------------------------------------------- VGS scenes, rows pinned to the oracle
SCENES = [
    ("urban", 120_000, dict(voxel_size=0.1)),
    ("pc", 60_000, dict(voxel_size=0.05, graph_size=0.25)),
    ("town", 80_000, dict()),
]


@pytest.mark.parametrize("scene", SCENES, ids=[s[0] for s in SCENES])
def test_vgs_graph(gpu, oracle, scene):
    name, n, kw = scene
    xyz = {"urban": gpu.scenes.urban_scene, "pc": gpu.scenes.pc_scene, "town": gpu.scenes.town_scene}[name](n)
    eng = _vgs(gpu, xyz, **kw)
    # the rows the truth is built from: the oracle's adjacency lists, used nodes only, equal the engine's vgs_get_lists(0)
    ref = oracle.run_vgs(xyz, oracle_params(oracle, eng.params))
    used = np.nonzero(ref.nodes()["used"])[0]
    ro, ri = ref.lists("adjacency")
    go, gi = eng.lists("adjacency")
    rs, gs = ragged_sets(ro, ri), ragged_sets(go, gi)
    uset = set(used.tolist())
    for v in used.tolist():
        assert {x for x in rs[v] if x in uset} == {x for x in gs[v] if x in uset}, v
    got = check_graph(eng)
    assert got["seg_ab"].shape[0] > 0
    check_boxes(eng, got)


def _svgs_rows_brute_force(eng):
    """SVGS: the stored rows equal a float32 radius search over the supervoxel centroids."""
    c = eng.attributes()["centroid"]
    gs = np.float32(eng.params.graph_size)
    r2 = np.float32(np.float64(gs) * np.float64(gs))
    off, idx = eng.lists("adjacency")
    V = c.shape[0]
    for i0 in range(0, V, 512):
        d = c[i0:i0 + 512, None, :] - c[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        for k in range(d2.shape[0]):
            want = np.nonzero(d2[k] < r2)[0]
            assert np.array_equal(np.sort(idx[off[i0 + k]:off[i0 + k + 1]]), want), i0 + k


@pytest.mark.parametrize("vccs_mode", [1, 0], ids=["pcl_order", "synchronous"])
def test_svgs_graph(gpu, vccs_mode):
    xyz = gpu.scenes.urban_scene(150_000)
    eng = gpu.Engine(gpu.default_params(3, vccs_mode=vccs_mode))
    eng.set_points(xyz)
    eng.run()
    _svgs_rows_brute_force(eng)
    got = check_graph(eng)
    assert got["seg_ab"].shape[0] > 0
    check_boxes(eng, got)


def test_svgs_graph_from_caller_labels(gpu):
    xyz = gpu.scenes.pc_scene(60_000)
    g = np.floor(xyz / 0.25).astype(np.int64)
    g -= g.min(axis=0)
    _, inv = np.unique(g[:, 0] * 1_000_003 + g[:, 1] * 1009 + g[:, 2], return_inverse=True)
    labels = (inv.reshape(-1) + 1).astype(np.int32)
    eng = gpu.Engine(gpu.default_params(3))
    eng.set_points(xyz)
    eng.set_supervoxel_labels(labels, int(labels.max()) + 1)
    eng.svgs_segment()
    got = check_graph(eng)
    assert got["seg_ab"].shape[0] > 0


# ---------------------------------------------------------------- a large scene: counts exact, weights on a seeded sample
def test_large_urban_scene(gpu):
    xyz = gpu.scenes.urban_scene(2_000_000)
    eng = _vgs(gpu, xyz, voxel_size=0.1)
    got = check_graph(eng, sample=300)
    assert got["seg_ab"].shape[0] > 300
    check_boxes(eng, got)


# ---------------------------------------------------------------- separate objects on a ground plane
def objects_on_ground(seed=3, side=16.0, step=0.04, pitch=4.0, radius=0.4, height=2.0, wall_step=0.03):
    """A flat ground and a grid of upright cylinders standing on it, dense enough that every voxel is used; the cylinders are
    pitch - 2 radius = 3.2 m apart (> graph_size)."""
    rng = np.random.default_rng(seed)
    g = np.arange(0.0, side, step)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    ground = np.stack([gx.ravel(), gy.ravel(), rng.normal(0.0, 0.003, gx.size)], axis=1)
    objs, owner = [], []
    centres = [(x, y) for x in np.arange(2.0, side - 1.0, pitch) for y in np.arange(2.0, side - 1.0, pitch)]
    n_ang, n_h = int(2 * np.pi * radius / wall_step), int(height / wall_step)
    for i, (cx, cy) in enumerate(centres):
        t, z = np.meshgrid(np.linspace(0, 2 * np.pi, n_ang, endpoint=False), np.linspace(0.02, height, n_h), indexing="ij")
        p = np.stack([cx + radius * np.cos(t).ravel(), cy + radius * np.sin(t).ravel(), z.ravel()], axis=1)
        p += rng.normal(0.0, 0.003, p.shape)
        objs.append(p)
        owner.append(np.full(p.shape[0], i))
    xyz = np.concatenate([ground] + objs).astype(np.float32)
    who = np.concatenate([np.full(ground.shape[0], -1)] + owner)   # -1: ground
    return xyz, who, len(centres)


def test_objects_on_ground(gpu):
    xyz, who, n_obj = objects_on_ground()
    eng = _vgs(gpu, xyz)
    got = check_graph(eng)
    check_boxes(eng, got)
    labels = eng.point_labels()
    K = eng.counts()["kept"]
    m = labels >= 0
    # per segment: which objects and whether the ground hold its points
    has = np.zeros((K, n_obj + 1), dtype=bool)
    has[labels[m], who[m] + 1] = True
    ground_seg = has[:, 0]
    obj_of = np.where(has[:, 1:].sum(axis=1) == 1, np.argmax(has[:, 1:], axis=1), -1)
    pure = ~ground_seg & (obj_of >= 0)   # segments of one object only
    a, b = got["seg_ab"][:, 0], got["seg_ab"][:, 1]
    both = pure[a] & pure[b]
    assert both.any()
    assert (obj_of[a][both] == obj_of[b][both]).all(), "an edge joins segments of different objects"
    # the ground is adjacent to every object: an edge between a segment holding ground points and a segment holding points of the object
    for i in range(n_obj):
        mine = has[:, i + 1] & ~ground_seg
        assert mine.any(), i
        touch = (mine[a] & ground_seg[b]) | (mine[b] & ground_seg[a])
        assert touch.any(), i


# ---------------------------------------------------------------- determinism, state, side effects
def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in FIELDS)


def test_deterministic(gpu):
    xyz = gpu.scenes.urban_scene(400_000)
    e1 = _vgs(gpu, xyz, voxel_size=0.1)
    a = e1.segment_graph()
    assert a["seg_ab"].shape[0] > 0
    assert _same(a, e1.segment_graph())
    e2 = _vgs(gpu, xyz, voxel_size=0.1)
    e2.run()
    assert _same(a, e2.segment_graph())


def test_state_contract(gpu):
    xyz = gpu.scenes.town_scene(60_000)
    eng = gpu.Engine(gpu.default_params(2))
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_graph()
    assert e.value.status == gpu._lib.VGS_E_STATE
    eng.set_points(xyz)
    eng.voxelize(); eng.features(); eng.adjacency()
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_graph()
    assert e.value.status == gpu._lib.VGS_E_STATE
    eng.segment()
    a = check_graph(eng)
    # a second cloud on the same engine: its own graph, not the cached one
    xyz2 = gpu.scenes.urban_scene(80_000)
    eng.set_points(xyz2)
    with pytest.raises(gpu.VgsError):
        eng.segment_graph()
    eng.run()
    b = check_graph(eng)
    assert a["seg_ab"].shape != b["seg_ab"].shape or not np.array_equal(a["seg_ab"], b["seg_ab"])
    # new parameters: the cache follows the new segmentation
    eng.set_params(gpu.default_params(2, cut_thred=0.5))
    eng.run()
    check_graph(eng)
    # no kept segment, and a single one: E = 0
    e0 = _vgs(gpu, xyz, voxels_min=10_000_000)
    assert e0.counts()["kept"] == 0
    g0 = e0.segment_graph()
    assert all(g0[k].shape[0] == 0 for k in FIELDS)
    rng = np.random.default_rng(1)
    blob = rng.normal(0.0, 0.3, size=(20_000, 3)).astype(np.float32)
    e1 = _vgs(gpu, blob, cut_thred=0.0)
    if e1.counts()["kept"] == 1:
        g1 = e1.segment_graph()
        assert all(g1[k].shape[0] == 0 for k in FIELDS)
    # the size query: every array NULL, n_edges written
    n = C.c_int64(-1)
    eng._ck(eng._L.vgs_get_segment_graph(eng._h, C.byref(n), *([None] * 7)))
    assert n.value == eng.segment_graph()["seg_ab"].shape[0]


def test_tile_context_is_refused(gpu):
    xyz = gpu.scenes.town_scene(60_000)
    eng = gpu.Engine(gpu.default_params(2))
    eng.set_points(xyz)
    lo = np.array([-1e9, -1e9], dtype=np.float64)
    hi = np.array([1e9, 1e9], dtype=np.float64)
    eng._ck(eng._L.vgs_set_owned_region(eng._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    eng.run()
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_graph()
    assert e.value.status == gpu._lib.VGS_E_STATE
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_graph_device()
    assert e.value.status == gpu._lib.VGS_E_STATE


def test_no_side_effects_and_device_variant(gpu):
    xyz = gpu.scenes.urban_scene(150_000)

    def others(eng):
        off, idx = eng.clusters()
        roff, ridx = eng.clusters("reference")
        _, kept = eng.node_labels()
        d = eng.segment_descriptors()
        return [off, idx, roff, ridx, eng.point_labels(), kept] + [d[k] for k in sorted(d)]

    e1 = _vgs(gpu, xyz)
    before = others(e1)
    g1 = e1.segment_graph()
    after = others(e1)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, after))
    # ... and the other way round: a graph asked for after every other getter is the same
    e2 = _vgs(gpu, xyz)
    others(e2)
    assert _same(g1, e2.segment_graph())
    # the device variant holds the same bytes
    E, ptrs = e1.segment_graph_device()
    assert E == g1["seg_ab"].shape[0] > 0
    hip = C.CDLL("libamdhip64.so")
    for name, dt, w in gpu.Engine.GRAPH_FIELDS:
        h = np.zeros(E * w, dtype=dt)
        assert hip.hipMemcpy(h.ctypes.data_as(C.c_void_p), C.c_void_p(ptrs[name]), C.c_size_t(h.nbytes), 2) == 0   # DeviceToHost
        assert np.array_equal(h.view(np.uint8), g1[name].reshape(-1).view(np.uint8)), name


def test_class_getters(gpu):
    xyz = gpu.scenes.town_scene(60_000)
    s = gpu.VoxelBasedSegmentation(0.15)
    s.setInputCloud(xyz); s.getCloudPointNum(xyz); s.addPointsFromInputCloud()
    s.setVoxelSize(0.15, 10, 3, 3)
    s.setVoxelCenters(); s.calcualteVoxelCloudAttributes(xyz); s.findAllVoxelAdjacency(0.5)
    s.segmentVoxelCloudWithGraphModel(0.3, 0.2, 0.2, 0.2, 0.2, 0.2, 2.0)
    assert s.getClusterGraph()["seg_ab"].shape == (0, 2)   # before drawColorMapofPointsinClusters, like getClusterIdx
    s.drawColorMapofPointsinClusters()
    g = s.getClusterGraph()
    assert _same(g, s.engine.segment_graph())
    # labels are getClusterIdx indices: an edge's clusters hold points within reach of each other
    idx = s.getClusterIdx()
    assert g["seg_ab"].max() < len(idx)
