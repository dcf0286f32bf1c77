"""Oriented bounding boxes of the kept segments (vgs_get_segment_boxes, csrc/segbox.hip) in both frames:
  * lo3, hi3, half3, center3 equal to tests/segment_boxes_ref.py (numpy float64, the header's association) by value, without a tolerance,
    on small scenes at the structural edges of the pass: chunk boundaries, nodes split across chunks, more segments than chunks,
    degenerate covariances, coordinates far from the origin, supervoxel nodes;
  * the frames: principal = evecs9 byte for byte; upright = exact z axis, orthonormal, sign rule, ascending variance, diagonalising;
  * the box against the points without the reported lo / hi; exact identities of the upright z axis against bbox6; geometry of two planes;
  * one-point segments, determinism, the state contract, no side effects on the other getters, the device variant.
Scenes from tests/segment_scenes.py run with the parameter sets of tests/test_gpu_segment_limits.py.  two_tilted_planes gives nine
segments there (voxel_size = 0.1, defaults), one under GROUP (graph_size 0.5 reaches over the 0.45 m gap) and one per voxel under SPLIT,
so the two planes as two segments come from PLANES = GROUP with graph_size = 0.3: below the gap, above the lattice pitch."""
import ctypes as C

import numpy as np
import pytest

from segment_boxes_ref import project, ref_boxes
from segment_scenes import FAR, GROUP, big_nodes, degenerate_scene, thin_segment, two_tilted_planes

pytestmark = pytest.mark.gpu

FRAMES = ("principal", "upright")
PLANES = dict(GROUP, graph_size=0.3)
BOX_KEYS = ("center3", "half3", "frame9", "lo3", "hi3")


def _engine(gpu, xyz, method=2, **kw):
    eng = gpu.Engine(gpu.default_params(method, **kw))
    eng.set_points(xyz)
    eng.run()
    return eng


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


SCENES = {
    "big_nodes": lambda gpu: (big_nodes(), 2, GROUP),
    "degenerate": lambda gpu: (degenerate_scene()[0], 2, GROUP),
    "degenerate_far": lambda gpu: (degenerate_scene(FAR)[0], 2, GROUP),
    "thin_far": lambda gpu: (thin_segment(), 2, GROUP),
    "tilted_planes_limits": lambda gpu: (two_tilted_planes(), 2, dict(voxel_size=0.1)),
    "tilted_planes": lambda gpu: (two_tilted_planes(), 2, PLANES),
    "town": lambda gpu: (gpu.scenes.town_scene(60_000), 2, {}),
    "pc_svgs": lambda gpu: (gpu.scenes.pc_scene(60_000), 3, {}),
}
_cache = {}


def _scene(gpu, name):
    """(points, segmented engine) of a scene, made once and shared; the tests that use it leave it segmented and unchanged."""
    if name not in _cache:
        xyz, method, kw = SCENES[name](gpu)
        _cache[name] = (xyz, _engine(gpu, xyz, method, **kw))
    return _cache[name]


def _check_frame(b, d, frame):
    K = d["n_points"].shape[0]
    W = b["frame9"].reshape(K, 3, 3)   # [k, r, j] = component r of axis j
    if frame == "principal":
        assert np.array_equal(b["frame9"].view(np.uint8), d["evecs9"].view(np.uint8))
    else:
        assert (W[:, :, 2] == np.array([0.0, 0.0, 1.0])).all()
        assert (W[:, 2, :2] == 0).all() and not np.signbit(W[:, 2, :2]).any()
        xx, xy, yy = d["cov6"][:, 0], d["cov6"][:, 1], d["cov6"][:, 3]
        Cm = np.stack([np.stack([xx, xy], axis=1), np.stack([xy, yy], axis=1)], axis=1)
        u = W[:, :2, :2]
        v = np.einsum("kri,krs,ksj->kij", u, Cm, u)
        tol = 1e-8 * (xx + yy) + 1e-30   # the form helpers.check_descriptors uses for cov6; the rotation's own error is a few ulp of xx + yy
        assert (np.abs(v[:, 0, 1]) <= tol).all()
        assert (v[:, 0, 0] <= v[:, 1, 1] + tol).all()
        ident = (xy == 0) & (xx <= yy)
        assert (W[ident] == np.eye(3)).all()
    assert np.allclose(np.einsum("kri,krj->kij", W, W), np.eye(3)[None], atol=1e-10)
    for j in range(3):
        col = W[:, :, j]
        assert (col[np.arange(K), np.argmax(np.abs(col), axis=1)] > 0).all(), j   # argmax: the lowest index on a tie


def _check_boxes(eng, xyz, frame):
    K = eng.counts()["kept"]
    b = eng.segment_boxes(frame)
    d = eng.segment_descriptors()
    labels = eng.point_labels()
    assert K > 0 and labels.max() == K - 1
    assert all(b[k].shape == (K, w) and b[k].dtype == np.float64 for k, _, w in eng.BOX_FIELDS)
    _check_frame(b, d, frame)
    # exact against the numpy restatement, from the engine's own centroid and frame
    ref = ref_boxes(xyz, labels, K, d["centroid3"], b["frame9"])
    for k in ("lo3", "hi3", "half3", "center3"):
        bad = np.nonzero(~(b[k] == ref[k]).all(axis=1))[0]
        assert bad.size == 0, (frame, k, bad[:5], b[k][bad[:5]], ref[k][bad[:5]])
    # the box against the points without the reported lo / hi: centre and half extent only.  mid = (min + max) / 2 and half = (max - min) / 2
    # round once each, so |t - mid| <= half holds to within an ulp of the extent (exactly when min + max is exact), and each face is reached
    m = labels >= 0
    lab = labels[m].astype(np.int64)
    t = project(xyz[m], d["centroid3"][lab], b["frame9"][lab])
    order = np.argsort(lab, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=K))[:-1]])
    tmin, tmax = np.minimum.reduceat(t[order], starts, axis=0), np.maximum.reduceat(t[order], starts, axis=0)
    mid = (tmin + tmax) * 0.5
    ulp = 2 * np.spacing(np.maximum(np.abs(tmin), np.abs(tmax)))
    off = np.abs(t - mid[lab])
    assert (off <= (b["half3"] + ulp)[lab]).all()
    reach_hi = np.zeros((K, 3), dtype=bool)
    reach_lo = np.zeros((K, 3), dtype=bool)
    np.logical_or.at(reach_hi, lab, (t - mid[lab]) >= (b["half3"] - ulp)[lab])
    np.logical_or.at(reach_lo, lab, (mid[lab] - t) >= (b["half3"] - ulp)[lab])
    assert reach_hi.all() and reach_lo.all()
    # the centre is the middle of the box: its own projection against mid, to the rounding of coordinates of the centroid's size and the
    # orthonormality bar of the frame (1e-10 per entry of W^T W)
    ct = project(b["center3"], d["centroid3"], b["frame9"])
    scale = np.abs(d["centroid3"]).max(axis=1) + np.abs(b["center3"]).max(axis=1) + 1.0
    assert (np.abs(ct - mid) <= (32 * np.finfo(np.float64).eps * scale + 3e-10 * np.abs(mid).max(axis=1))[:, None]).all()
    if frame == "upright":
        # (0 dx + 0 dy) + 1 dz is dz: the z bounds are the float box against the centroid, exactly
        assert (b["lo3"][:, 2] == d["bbox6"][:, 2].astype(np.float64) - d["centroid3"][:, 2]).all()
        assert (b["hi3"][:, 2] == d["bbox6"][:, 5].astype(np.float64) - d["centroid3"][:, 2]).all()
    one = d["n_points"] == 1
    assert (b["half3"][one] == 0).all() and (b["lo3"][one] == 0).all() and (b["hi3"][one] == 0).all()
    return b, d, labels


# ---------------------------------------------------------------- exactness, frames, containment on every scene
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", list(SCENES))
def test_boxes_equal_the_numpy_restatement(gpu, name, frame):
    xyz, eng = _scene(gpu, name)
    _check_boxes(eng, xyz, frame)


def test_scenes_reach_their_edges(gpu):
    """The scenes hold what they are named for: segments just below, on and above chunk multiples; more segments than chunks; one-point segments."""
    from helpers import SD_CHUNK
    _, eng = _scene(gpu, "big_nodes")
    n = eng.segment_descriptors()["n_points"]
    assert {0, 1, SD_CHUNK - 1} <= set((n % SD_CHUNK).tolist()) and n.max() >= 10_000 and (n == 1).any()
    xyz, eng = _scene(gpu, "degenerate")
    assert eng.counts()["kept"] > xyz.shape[0] // SD_CHUNK + 1
    _, eng = _scene(gpu, "pc_svgs")
    assert eng.counts()["supervoxels"] > 0


# ---------------------------------------------------------------- geometry of two planes
def test_two_tilted_planes_principal(gpu):
    xyz, eng = _scene(gpu, "tilted_planes")
    assert eng.counts()["kept"] == 2                      # PLANES: each plane one segment
    d = eng.segment_descriptors()
    assert d["n_points"].tolist() == [25_600, 25_600]     # 12.5 chunks each
    b = eng.segment_boxes("principal")
    ext = 2 * b["half3"]
    assert (ext[:, 0] <= 1e-5).all(), ext                 # along the normal: float32 rounding of coordinates <= 4 m is 2.4e-7
    assert (ext[:, 1:] >= 3.975).all(), ext               # the lattice's side, in both in-plane axes


# ---------------------------------------------------------------- one-point segments
@pytest.mark.parametrize("frame", FRAMES)
def test_one_point_segments(gpu, frame):
    seen = 0
    for name in ("big_nodes", "degenerate"):
        xyz, eng = _scene(gpu, name)
        b, d, labels = eng.segment_boxes(frame), eng.segment_descriptors(), eng.point_labels()
        one = np.nonzero(d["n_points"] == 1)[0]
        assert one.size >= 1
        for k in one.tolist():
            p = xyz[labels == k][0].astype(np.float64)
            assert (b["half3"][k] == 0).all() and (b["lo3"][k] == 0).all() and (b["hi3"][k] == 0).all()
            assert (b["center3"][k] == p).all()
            seen += 1
    assert seen >= 2


# ---------------------------------------------------------------- determinism
def test_deterministic(gpu):
    xyz, e1 = _scene(gpu, "big_nodes")
    a = {f: e1.segment_boxes(f) for f in FRAMES}
    for f in FRAMES:
        assert _same(a[f], e1.segment_boxes(f))          # call to call (the cache)
    e2 = _engine(gpu, xyz, **GROUP)
    for f in reversed(FRAMES):
        assert _same(a[f], e2.segment_boxes(f))          # engine to engine
    e2.run()
    for f in FRAMES:
        assert _same(a[f], e2.segment_boxes(f))          # after a re-run (computed again)


# ---------------------------------------------------------------- state contract
def test_state_contract(gpu):
    xyz = gpu.scenes.town_scene(60_000)
    eng = gpu.Engine(gpu.default_params(2))
    for f in FRAMES:
        with pytest.raises(gpu.VgsError) as e:
            eng.segment_boxes(f)
        assert e.value.status == gpu._lib.VGS_E_STATE
    eng.set_points(xyz)
    eng.voxelize(); eng.features(); eng.adjacency()
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_boxes_device("upright")
    assert e.value.status == gpu._lib.VGS_E_STATE
    eng.segment()
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_boxes(2)
    assert e.value.status == gpu._lib.VGS_E_ARG
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_boxes_device(-1)
    assert e.value.status == gpu._lib.VGS_E_ARG
    a = {f: _check_boxes(eng, xyz, f)[0] for f in FRAMES}
    # a second cloud on the same engine: refused until the next run, then its own boxes
    xyz2 = gpu.scenes.urban_scene(40_000)
    eng.set_points(xyz2)
    for f in FRAMES:
        with pytest.raises(gpu.VgsError) as e:
            eng.segment_boxes(f)
        assert e.value.status == gpu._lib.VGS_E_STATE
    eng.run()
    for f in FRAMES:
        b = _check_boxes(eng, xyz2, f)[0]
        assert b["lo3"].shape != a[f]["lo3"].shape or not np.array_equal(b["lo3"], a[f]["lo3"])
    # new parameters and a run: the boxes follow the new labels
    la = eng.point_labels()
    eng.set_params(gpu.default_params(2, cut_thred=0.5))
    eng.run()
    assert not np.array_equal(la, eng.point_labels())
    for f in FRAMES:
        _check_boxes(eng, xyz2, f)
    # no kept segment: empty arrays
    e0 = _engine(gpu, xyz, voxels_min=10_000_000)
    assert e0.counts()["kept"] == 0
    for f in FRAMES:
        b0 = e0.segment_boxes(f)
        assert sorted(b0) == sorted(BOX_KEYS) and all(b0[k].shape == (0, w) for k, _, w in e0.BOX_FIELDS)


def test_tile_context_is_refused(gpu):
    xyz = gpu.scenes.town_scene(60_000)
    eng = gpu.Engine(gpu.default_params(2))
    eng.set_points(xyz)
    lo = np.array([-1e9, -1e9], dtype=np.float64)
    hi = np.array([1e9, 1e9], dtype=np.float64)
    eng._ck(eng._L.vgs_set_owned_region(eng._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    eng.run()
    for f in FRAMES:
        with pytest.raises(gpu.VgsError) as e:
            eng.segment_boxes(f)
        assert e.value.status == gpu._lib.VGS_E_STATE


def test_class_mirror(gpu):
    """getClusterBoxes of both classes: empty where getClusterDescriptors is, the engine's table afterwards; a state error before segmentation."""
    xyz = gpu.scenes.town_scene(60_000)
    s = gpu.VoxelBasedSegmentation(0.15)
    s.setInputCloud(xyz); s.getCloudPointNum(xyz); s.addPointsFromInputCloud()
    s.setVoxelSize(0.15, 10, 3, 3)
    s.setVoxelCenters(); s.calcualteVoxelCloudAttributes(xyz); s.findAllVoxelAdjacency(0.5)
    s.segmentVoxelCloudWithGraphModel(0.3, 0.2, 0.2, 0.2, 0.2, 0.2, 2.0)
    e = s.getClusterBoxes()
    assert sorted(e) == sorted(BOX_KEYS) and all(v.shape[0] == 0 for v in e.values()) and s.getClusterDescriptors()["n_points"].shape[0] == 0
    s.drawColorMapofPointsinClusters()
    for f in FRAMES:
        assert _same(s.getClusterBoxes(frame=f), s.engine.segment_boxes(f))
    assert s.getClusterBoxes()["lo3"].shape[0] == len(s.getClusterIdx()) > 0
    v = gpu.SuperVoxelBasedSegmentation(0.05)
    v.setInputCloud(xyz); v.addPointsFromInputCloud()
    with pytest.raises(gpu.VgsError) as err:
        v.getClusterBoxes()
    assert err.value.status == gpu._lib.VGS_E_STATE


# ---------------------------------------------------------------- no side effects
def _others(eng):
    off, idx = eng.clusters()
    vt = eng.voxel_table()
    at = eng.attributes()
    d = eng.segment_descriptors()
    g = eng.segment_graph()
    return ([off, idx, eng.point_labels(), vt["key"], vt["start"], vt["point_idx"]] + [at[k] for k in sorted(at)] + [d[k] for k in sorted(d)] +
            [g[k] for k in sorted(g)])


def _eq(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_no_side_effects(gpu):
    xyz = gpu.scenes.town_scene(60_000)
    e1 = _engine(gpu, xyz)
    before = _others(e1)
    b1 = {f: e1.segment_boxes(f) for f in FRAMES}
    assert _eq(before, _others(e1))
    # the other way round: boxes asked for first, before any other getter (the descriptor table is computed on the way)
    e2 = _engine(gpu, xyz)
    b2 = {f: e2.segment_boxes(f) for f in reversed(FRAMES)}
    assert all(_same(b1[f], b2[f]) for f in FRAMES)
    assert _eq(before, _others(e2))
    # vgs_segment_descriptors_from_moments overwrites the descriptor buffers of the context: the cached boxes keep their bytes and their
    # frame, and the context's own descriptors come back as they were
    one = dict(n=np.array([4], np.int64), nodes=np.array([1], np.int32), box=np.array([0, 0, 0, 1, 2, 3], np.float32),
               anc=np.array([5, 6, 7], np.float32), s9=np.array([1, 2, 3, 9, 1, 2, 8, 3, 7], np.float64))
    ev = np.zeros(9, np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    e1._ck(e1._L.vgs_segment_descriptors_from_moments(e1._h, 1, p(one["n"]), p(one["nodes"]), p(one["box"]), p(one["anc"]), p(one["s9"]),
                                                      None, None, None, None, None, None, p(ev), None))
    assert np.abs(ev).sum() > 0
    assert all(_same(b1[f], e1.segment_boxes(f)) for f in FRAMES)
    assert _eq(before, _others(e1))
    # ... and a box table computed after such a call is the same as well
    e3 = _engine(gpu, xyz)
    e3._ck(e3._L.vgs_segment_descriptors_from_moments(e3._h, 1, p(one["n"]), p(one["nodes"]), p(one["box"]), p(one["anc"]), p(one["s9"]),
                                                      None, None, None, None, None, None, None, None))
    assert all(_same(b1[f], e3.segment_boxes(f)) for f in FRAMES)


# ---------------------------------------------------------------- device variant
def test_device_variant_and_device_points(gpu):
    torch = pytest.importorskip("torch")
    xyz = gpu.scenes.town_scene(60_000)
    e1 = _engine(gpu, xyz)
    hip = C.CDLL("libamdhip64.so")
    host = {}
    for f in FRAMES:
        ptrs = e1.segment_boxes_device(f)      # computes the table; the host variant then copies the same buffers
        host[f] = e1.segment_boxes(f)
        K = host[f]["lo3"].shape[0]
        assert K > 0
        for name, dt, w in gpu.Engine.BOX_FIELDS:
            h = np.zeros(K * w, dtype=dt)
            assert hip.hipMemcpy(h.ctypes.data_as(C.c_void_p), C.c_void_p(ptrs[name]), C.c_size_t(h.nbytes), 2) == 0   # DeviceToHost
            assert np.array_equal(h.view(np.uint8), host[f][name].reshape(-1).view(np.uint8)), (f, name)
    assert len({e1.segment_boxes_device(f)["lo3"] for f in FRAMES}) == 2   # both frames cached at once, in buffers of their own
    dev = torch.from_numpy(xyz).to("cuda:0")
    torch.cuda.synchronize()
    e2 = gpu.Engine(gpu.default_params(2))
    e2.set_points_device(dev.data_ptr(), xyz.shape[0], 12, keep=dev)
    e2.run()
    for f in FRAMES:
        assert _same(host[f], e2.segment_boxes(f))
