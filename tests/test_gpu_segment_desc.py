"""Per-segment descriptors (vgs_get_segment_descriptors, csrc/segdesc.hip) against numpy float64 of the same float32 points: counts,
exact boxes, two-pass centroid and covariance, eigh, the sign rule and the eight eigen features -- for VGS, for SVGS (PCL-order, the
synchronous variant and a caller's labelling), for a large plane among many small segments near and far from the origin; plus determinism,
the call-state contract and the absence of side effects on the other getters."""
import ctypes as C

import numpy as np
import pytest

from helpers import check_descriptors

pytestmark = pytest.mark.gpu


def _vgs(gpu, xyz, **kw):
    eng = gpu.Engine(gpu.default_params(2, **kw))
    eng.set_points(xyz)
    eng.run()
    return eng


# ---------------------------------------------------------------- VGS and SVGS scenes
@pytest.mark.parametrize("scene", [("urban", 150_000), ("pc", 60_000), ("town", None)], ids=["urban", "pc", "town"])
def test_vgs_descriptors(gpu, scene):
    name, n = scene
    f = {"urban": gpu.scenes.urban_scene, "pc": gpu.scenes.pc_scene, "town": gpu.scenes.town_scene}[name]
    xyz = f(n) if n else f()
    eng = _vgs(gpu, xyz)
    check_descriptors(eng, xyz, svgs=False)
    # the node count matches the voxels behind the points as well
    pv, labels = eng.point_voxel(), eng.point_labels()
    _, kept = eng.node_labels()
    inside = pv >= 0
    assert np.array_equal(labels[inside], kept[pv[inside]])


@pytest.mark.parametrize("vccs_mode", [1, 0], ids=["pcl_order", "synchronous"])
def test_svgs_descriptors(gpu, vccs_mode):
    xyz = gpu.scenes.urban_scene(150_000)
    eng = gpu.Engine(gpu.default_params(3, vccs_mode=vccs_mode))
    eng.set_points(xyz)
    eng.run()
    check_descriptors(eng, xyz, svgs=True)


def test_svgs_descriptors_from_caller_labels(gpu):
    xyz = gpu.scenes.pc_scene(60_000)
    g = np.floor(xyz / 0.25).astype(np.int64)
    g -= g.min(axis=0)
    _, inv = np.unique(g[:, 0] * 1_000_003 + g[:, 1] * 1009 + g[:, 2], return_inverse=True)
    labels = (inv.reshape(-1) + 1).astype(np.int32)
    eng = gpu.Engine(gpu.default_params(3))
    eng.set_points(xyz)
    eng.set_supervoxel_labels(labels, int(labels.max()) + 1)
    eng.svgs_segment()
    check_descriptors(eng, xyz, svgs=True)


# ---------------------------------------------------------------- one large plane among many small blobs
NORMAL = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
SIGMA = 0.005


def plane_and_blobs(seed=7, n_plane=2_100_000, n_blobs=1200, per_blob=200):
    rng = np.random.default_rng(seed)
    u = np.cross(NORMAL, [1.0, 0.0, 0.0]); u /= np.linalg.norm(u)
    v = np.cross(NORMAL, u)
    st = rng.uniform(-20.0, 20.0, size=(n_plane, 2))
    plane = st[:, :1] * u + st[:, 1:] * v + rng.normal(0.0, SIGMA, size=(n_plane, 1)) * NORMAL
    cen = np.stack([rng.uniform(-18, 18, n_blobs), rng.uniform(-18, 18, n_blobs), np.zeros(n_blobs)], axis=1)
    cen[:, 2] = -(NORMAL[0] * cen[:, 0] + NORMAL[1] * cen[:, 1]) / NORMAL[2] + rng.uniform(3.0, 8.0, n_blobs)
    blobs = (cen[:, None, :] + rng.normal(0.0, 0.06, size=(n_blobs, per_blob, 3))).reshape(-1, 3)
    return plane.astype(np.float32), blobs.astype(np.float32)


@pytest.fixture(scope="module")
def plane_scene(gpu):
    plane, blobs = plane_and_blobs()
    xyz = np.concatenate([plane, blobs])
    return xyz, plane.shape[0]


def test_large_plane_among_small_blobs(gpu, plane_scene):
    xyz, n_plane = plane_scene
    eng = _vgs(gpu, xyz)
    got = check_descriptors(eng, xyz, svgs=False)
    labels = eng.point_labels()
    pl = labels[:n_plane]
    k = int(np.bincount(pl[pl >= 0]).argmax())
    assert got["n_points"][k] > 500_000
    assert eng.counts()["kept"] > 300   # many small segments beside the plane in the same call
    nrm = got["evecs9"][k].reshape(3, 3)[:, 0]
    ang = np.arccos(min(1.0, abs(float(nrm @ NORMAL))))
    assert ang <= 1e-4, ang
    assert abs(got["evals3"][k, 0] / SIGMA ** 2 - 1) <= 0.05, got["evals3"][k, 0]


def test_far_from_origin(gpu, plane_scene):
    xyz, _ = plane_scene
    far = (xyz.astype(np.float64) + np.array([3e5, 5e5, 50.0])).astype(np.float32)
    eng = _vgs(gpu, far)
    check_descriptors(eng, far, svgs=False)


# ---------------------------------------------------------------- determinism, state, side effects
def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def test_deterministic(gpu, plane_scene):
    xyz, _ = plane_scene
    e1 = _vgs(gpu, xyz)
    a = e1.segment_descriptors()
    assert _same(a, e1.segment_descriptors())
    e2 = _vgs(gpu, xyz)
    e2.run()
    assert _same(a, e2.segment_descriptors())


def test_state_contract(gpu):
    xyz = gpu.scenes.town_scene(60_000)
    eng = gpu.Engine(gpu.default_params(2))
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_descriptors()
    assert e.value.status == gpu._lib.VGS_E_STATE
    eng.set_points(xyz)
    eng.voxelize(); eng.features(); eng.adjacency()
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_descriptors()
    assert e.value.status == gpu._lib.VGS_E_STATE
    eng.segment()
    a = check_descriptors(eng, xyz, svgs=False)
    # a second cloud on the same engine: its own descriptors, not the cached ones
    xyz2 = gpu.scenes.urban_scene(80_000)
    eng.set_points(xyz2)
    with pytest.raises(gpu.VgsError):
        eng.segment_descriptors()
    eng.run()
    b = check_descriptors(eng, xyz2, svgs=False)
    assert a["n_points"].shape != b["n_points"].shape or not np.array_equal(a["n_points"], b["n_points"])
    # new parameters: the cache follows the new segmentation
    p = gpu.default_params(2, cut_thred=0.5)
    eng.set_params(p)
    eng.run()
    check_descriptors(eng, xyz2, svgs=False)
    # no kept segment: empty arrays
    e0 = _vgs(gpu, xyz, voxels_min=10_000_000)
    assert e0.counts()["kept"] == 0
    d0 = e0.segment_descriptors()
    assert all(v.shape[0] == 0 for v in d0.values())


def test_tile_context_is_refused(gpu):
    xyz = gpu.scenes.town_scene(60_000)
    eng = gpu.Engine(gpu.default_params(2))
    eng.set_points(xyz)
    lo = np.array([-1e9, -1e9], dtype=np.float64)
    hi = np.array([1e9, 1e9], dtype=np.float64)
    eng._ck(eng._L.vgs_set_owned_region(eng._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    eng.run()
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_descriptors()
    assert e.value.status == gpu._lib.VGS_E_STATE


def test_no_side_effects(gpu):
    xyz = gpu.scenes.urban_scene(150_000)

    def others(eng):
        off, idx = eng.clusters()
        roff, ridx = eng.clusters("reference")
        vt = eng.voxel_table()
        at = eng.attributes()
        return [off, idx, roff, ridx, eng.point_labels(), vt["key"], vt["start"], vt["point_idx"]] + [at[k] for k in sorted(at)]

    e1 = _vgs(gpu, xyz)
    before = others(e1)
    d1 = e1.segment_descriptors()
    after = others(e1)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # ... and the other way round: descriptors asked for after every other getter are the same
    e2 = _vgs(gpu, xyz)
    others(e2)
    assert _same(d1, e2.segment_descriptors())
    assert _same(d1, e1.segment_descriptors())


def test_device_variant_and_device_points(gpu):
    torch = pytest.importorskip("torch")
    xyz = gpu.scenes.town_scene(60_000)
    e1 = _vgs(gpu, xyz)
    d1 = e1.segment_descriptors()
    ptrs = e1.segment_descriptors_device()
    K = d1["n_points"].shape[0]
    hip = C.CDLL("libamdhip64.so")
    for name, dt, w in gpu.Engine.DESCRIPTOR_FIELDS:
        h = np.zeros(K * w, dtype=dt)
        assert hip.hipMemcpy(h.ctypes.data_as(C.c_void_p), C.c_void_p(ptrs[name]), C.c_size_t(h.nbytes), 2) == 0   # DeviceToHost
        assert np.array_equal(h.view(np.uint8), d1[name].reshape(-1).view(np.uint8)), name
    dev = torch.from_numpy(xyz).to("cuda:0")
    torch.cuda.synchronize()
    e2 = gpu.Engine(gpu.default_params(2))
    e2.set_points_device(dev.data_ptr(), xyz.shape[0], 12, keep=dev)
    e2.run()
    assert _same(d1, e2.segment_descriptors())
