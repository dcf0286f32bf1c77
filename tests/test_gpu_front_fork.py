"""The front of vgs_run forks: the main stream builds the voxel table, the used flags (k_used_flags), their scan and compaction and the
brick table, then a side stream gathers the points into leaf order and runs k_features while the main stream builds the adjacency rows;
the main stream joins in front of the local cut.  Every array is computed by the same kernels from the same inputs on either route, so the forked
route is compared BIT FOR BIT with the serial one -- an engine created with VGS_NO_OVERLAP, which keeps every kernel of the front on one
stream -- array by array: voxel table, point -> voxel map, node attributes, adjacency counts and lists, node labels, point labels, counts.

The shapes are the smallest at which an ordering or aliasing mistake can show:
  empty and degenerate fronts (no finite point, one point, no used voxel, one used voxel beside one just below points_min), each followed
      by a normal run on the same context: the early returns between fork and join must leave the side stream joined;
  non-finite points scattered through 50 k points: N_finite < N while the side stream gathers all N slots;
  the three key layouts: 32-bit keys, 64-bit keys with the index packed (k_run_counts unpacks the order the gather reads), 64-bit keys
      with the index as a value (two outliers 60 km apart bring depth 20: 61 key bits + 13 index bits);
  one context over clouds of differing size (200 k, 2 k, 200 k again): stale xs/ys/zs, node or perm_b of the cloud before would show;
  five runs of one context and a second engine; the single-stage entry points against run(); 200 k points against the CPU oracle."""
import os

import numpy as np
import pytest

from helpers import canonical_labels, oracle_params

pytestmark = pytest.mark.gpu

KW = dict(voxel_size=0.1)
POINTS_MIN = 10   # default_params(2)


def _engine(gpu, serial, **kw):
    """serial: created with VGS_NO_OVERLAP set (the knobs are read once, at creation)."""
    old = os.environ.get("VGS_NO_OVERLAP")
    if serial:
        os.environ["VGS_NO_OVERLAP"] = "1"
    else:
        os.environ.pop("VGS_NO_OVERLAP", None)
    try:
        return gpu.Engine(gpu.default_params(2, **(kw or KW)))
    finally:
        if old is None:
            os.environ.pop("VGS_NO_OVERLAP", None)
        else:
            os.environ["VGS_NO_OVERLAP"] = old


def _arrays(eng):
    c = eng.counts()
    out = {"counts": np.array([c[k] for k in ("points", "finite", "voxels", "used", "adj", "clusters", "kept", "depth", "isolated", "reattached")]),
           "point_labels": eng.point_labels().copy()}
    if c["voxels"] == 0:
        return out
    t = eng.voxel_table()
    out.update(key=t["key"], start=t["start"], point_idx=t["point_idx"], point_voxel=eng.point_voxel())
    a = eng.attributes()
    out.update({k: a[k].view(np.uint32 if a[k].dtype == np.float32 else a[k].dtype) for k in ("centroid", "normal", "eigen", "used")})
    out["adjacency_counts"] = eng.adjacency_counts()
    off, idx = eng.lists("adjacency")
    out.update(adj_off=off.copy(), adj_idx=idx.copy())
    root, kept = eng.node_labels()
    out.update(root=root, kept=kept)
    return out


def _same(a, b, what=""):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _run(eng, xyz):
    eng.set_points(xyz)
    eng.run()
    return _arrays(eng)


def plane(n=10_000, seed=5):
    """1 m x 1 m of a plane, 100 points per 0.1 m voxel: a normal run with used voxels and kept segments."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0.0, 1.0, (n, 3))
    xyz[:, 2] = rng.uniform(-0.002, 0.002, n)
    return xyz.astype(np.float32)


def _degenerate(name):
    rng = np.random.default_rng(11)
    if name == "no_finite":
        xyz = np.full((100, 3), np.nan, dtype=np.float32)
        xyz[::3, 1] = np.inf
        return xyz
    if name == "one_point":
        return np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    if name == "no_used":   # 500 points over 200^3 voxels: none holds more than points_min
        return rng.uniform(0.0, 20.0, (500, 3)).astype(np.float32)
    if name == "one_used":
        # points_min + 1 points in one voxel, points_min in the voxel beside it.  The octree's first box puts the first point at the upper
        # end of cell 0 on every axis (OctreeBox::adopt: min = p - res + eps / 2), so the clusters sit half a cell below it, well inside
        # cells (0, 0, 0) and (1, 0, 0); the first point itself lands in the first cluster's voxel or, by rounding, alone beside it
        p0 = np.array([[1.0, 1.0, 1.0]])
        a = p0 + [-0.05, -0.05, -0.05] + rng.uniform(-0.02, 0.02, (POINTS_MIN + 1, 3))
        b = p0 + [0.05, -0.05, -0.05] + rng.uniform(-0.02, 0.02, (POINTS_MIN, 3))
        rest = np.concatenate([a, b])[rng.permutation(2 * POINTS_MIN + 1)]
        return np.concatenate([p0, rest]).astype(np.float32)
    raise KeyError(name)


@pytest.fixture(scope="module")
def urban(gpu):
    """urban_scene(200_000) on the serial route (the reference of the tests below, left unchanged) and on the forked one."""
    xyz = gpu.scenes.urban_scene(200_000)
    ser = _run(_engine(gpu, True), xyz)
    eng = _engine(gpu, False)
    return dict(xyz=xyz, serial=ser, eng=eng, fork=_run(eng, xyz))


@pytest.mark.parametrize("name", ["no_finite", "one_point", "no_used", "one_used"])
def test_degenerate_front_then_a_normal_run(gpu, name):
    xyz, normal = _degenerate(name), plane()
    fork, ser = _engine(gpu, False), _engine(gpu, True)
    first = _run(fork, xyz)
    _same(first, _run(ser, xyz), name)
    c = dict(zip(("points", "finite", "voxels", "used"), first["counts"][:4]))
    want = {"no_finite": (0, 0, 0), "one_point": (1, 1, 0), "no_used": (500, None, 0), "one_used": (2 * POINTS_MIN + 2, None, 1)}[name]
    assert c["finite"] == want[0] and (want[1] is None or c["voxels"] == want[1]) and c["used"] == want[2], c
    if name == "one_used":
        sizes = np.sort(np.diff(first["start"]))
        assert sizes[-1] in (POINTS_MIN + 1, POINTS_MIN + 2) and sizes[-2] == POINTS_MIN and c["voxels"] in (2, 3), sizes
    second = _run(fork, normal)
    _same(second, _run(ser, normal), name + ", normal run behind it")
    assert second["counts"][3] >= 100 and second["counts"][6] > 0, second["counts"]   # used voxels, kept segments
    _same(_run(fork, xyz), first, name + " again")


def test_non_finite_points_scattered_through_the_cloud(gpu):
    xyz = gpu.scenes.urban_scene(50_000).copy()
    rng = np.random.default_rng(3)
    bad = rng.choice(xyz.shape[0], 4_000, replace=False)
    xyz[bad, rng.integers(0, 3, bad.size)] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), bad.size)
    f = _run(_engine(gpu, False), xyz)
    assert f["counts"][1] == xyz.shape[0] - bad.size and f["counts"][3] > 0, f["counts"]
    _same(f, _run(_engine(gpu, True), xyz))


def _layout(depth, n):
    """What voxelize_sorted_table chooses (as tests/test_gpu_voxel_runs.py states it)."""
    key_bits, idx_bits = 3 * depth + 1, 1
    while idx_bits < 32 and (1 << idx_bits) < n:
        idx_bits += 1
    return "u32" if key_bits <= 32 else ("u64-packed" if key_bits + idx_bits <= 64 else "u64")


@pytest.mark.parametrize("layout,far", [("u32", None), ("u64-packed", 250.0), ("u64", 60_000.0)])
def test_key_layouts(gpu, layout, far):
    """6 k points of a plane (used voxels, segments) and, for the 64-bit layouts, two outliers `far` metres from it along x and y."""
    xyz = plane(6_000, seed=7)
    if far:
        xyz = np.concatenate([xyz[:3000], [[far, 0.0, 0.0]], xyz[3000:], [[0.0, far, 0.0]]]).astype(np.float32)
    f = _run(_engine(gpu, False), xyz)
    assert _layout(int(f["counts"][7]), xyz.shape[0]) == layout, f["counts"]
    assert f["counts"][3] > 0 and f["counts"][6] > 0, f["counts"]
    _same(f, _run(_engine(gpu, True), xyz), layout)


def test_forked_route_equals_the_serial_one(urban):
    assert urban["fork"]["counts"][3] > 1000 and urban["fork"]["counts"][6] > 0, urban["fork"]["counts"]
    _same(urban["fork"], urban["serial"])


def test_one_context_over_differing_clouds(gpu, urban):
    small = gpu.scenes.urban_scene(2_000)
    small_ref = _run(_engine(gpu, True, voxel_size=0.1), small)
    eng = urban["eng"]                      # has run the 200 k cloud
    _same(_run(eng, small), small_ref, "2 k behind 200 k")
    _same(_run(eng, urban["xyz"]), urban["serial"], "200 k behind 2 k")
    _same(_run(eng, small), small_ref, "2 k again")


def test_five_runs_and_a_second_engine_repeat_the_arrays(gpu, urban):
    eng = urban["eng"]
    eng.set_points(urban["xyz"])
    for _ in range(5):
        eng.run()
        _same(_arrays(eng), urban["serial"])
    _same(_run(_engine(gpu, False), urban["xyz"]), urban["serial"], "second engine")


def test_single_stages_equal_run(gpu, urban):
    eng = _engine(gpu, False)
    eng.set_points(urban["xyz"])
    eng.voxelize(); eng.features(); eng.adjacency(); eng.segment()
    _same(_arrays(eng), urban["serial"])
    eng.run()                               # and the fork behind the single stages on the same context
    _same(_arrays(eng), urban["serial"])


def test_urban_200k_equals_the_oracle(gpu, oracle, urban):
    p = gpu.default_params(2, **KW)
    ref = oracle.run_vgs(urban["xyz"], oracle_params(oracle, p))
    f, r, n = urban["fork"], ref.voxel_table(), ref.nodes()
    assert (f["counts"][2], f["counts"][1]) == (ref.V, ref.n_finite)
    for k in ("key", "start", "point_idx", "point_voxel"):
        np.testing.assert_array_equal(f[k], r[k], err_msg=k)
    np.testing.assert_array_equal(f["used"], n["used"])
    for k in ("centroid", "normal", "eigen"):
        np.testing.assert_array_equal(f[k], n[k].view(np.uint32), err_msg=k)
    ro, ri = ref.lists("adjacency")
    np.testing.assert_array_equal(f["adj_off"], ro)
    np.testing.assert_array_equal(f["adj_idx"], ri)
    pl_ref, nc_ref = ref.labels()
    np.testing.assert_array_equal(canonical_labels(f["root"]), canonical_labels(nc_ref))
    np.testing.assert_array_equal(f["point_labels"], pl_ref)
