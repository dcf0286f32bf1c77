"""CPU tests of the host side: the C-ABI library loads and exports every symbol include/vgs.h declares,
parameter surface / task-file parsing (test:25-37, 108-125; point_clouds_IO.cpp:148-169), loud failure without a
GPU, scene determinism, schedule-bound properties of the lazy local cut."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(vgs):
    hdr = open(os.path.join(ROOT, "include", "vgs.h")).read()
    declared = set(re.findall(r"\b(s?vgs_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"vgs_status"}
    lib = C.CDLL(vgs._lib.LIB_PATH)
    missing = [n for n in sorted(declared) if not hasattr(lib, n)]
    assert not missing, missing
    bound = {n for n, _, _ in vgs._lib.SYMBOLS}
    assert declared == bound, (declared ^ bound)


def test_defaults_match_task_files(vgs):
    p = vgs.default_params(2)
    assert (p.method, p.points_min, p.adjacency_min, p.voxels_min) == (2, 10, 3, 3)
    assert np.float32(p.voxel_size) == np.float32(0.15) and np.float32(p.sig_w) == np.float32(2.0) and np.float32(p.cut_thred) == np.float32(0.3)
    s = vgs.default_params(3)
    assert s.method == 3 and np.float32(s.voxel_size) == np.float32(0.05) and np.float32(s.seed_size) == np.float32(0.25)
    assert np.float32(s.sig_w) == np.float32(1.0) and np.float32(s.cut_thred) == np.float32(0.5)
    assert (np.float32(s.color_impt), np.float32(s.spatial_impt), np.float32(s.normal_impt)) == (np.float32(0), np.float32(0.25), np.float32(0.75))
    assert s.vccs_mode == 1      # createSupervoxels calls pcl::SupervoxelClustering (SS:265-284): PCL's own order is the default


def _write_task(path, method, lines):
    body = ["// header"] * 70
    for k, v in lines.items():
        body[k] = str(v)
    body[24] = str(method)
    with open(path, "wb") as f:
        f.write("\r\n".join(body).encode())  # the reference's task files are CRLF


def test_parse_task_file_vgs(vgs, tmp_path):
    f = tmp_path / "Task_File_VGS.txt"
    _write_task(f, 2, {7: "Seg", 15: "Town_Test.pcd", 21: "Town_Test_VGS.pcd", 28: 0.15, 30: 0.5, 32: 0.2, 34: 0.21, 36: 0.22,
                       38: 0.23, 40: 0.24, 42: 2, 44: 0.3, 46: 10, 48: 3, 50: 4})
    p, inn, out = vgs.parse_task_file(str(f))
    assert (inn, out) == ("Town_Test.pcd", "Town_Test_VGS.pcd")
    assert p.method == 2 and (p.points_min, p.adjacency_min, p.voxels_min) == (10, 3, 4)
    got = [p.voxel_size, p.graph_size, p.sig_p, p.sig_n, p.sig_o, p.sig_e, p.sig_c, p.sig_w, p.cut_thred]
    np.testing.assert_array_equal(np.float32(got), np.float32([0.15, 0.5, 0.2, 0.21, 0.22, 0.23, 0.24, 2, 0.3]))


def test_parse_task_file_svgs(vgs, tmp_path):
    f = tmp_path / "Task_File_SVGS.txt"
    _write_task(f, 3, {15: "a.pcd", 21: "b.pcd", 28: 0.05, 30: 0.25, 32: 0.5, 34: 0.2, 36: 0.2, 38: 0.2, 40: 0.2, 42: 0.2, 44: 1,
                       46: 0, 48: 0.25, 50: 0.75, 52: 0.5, 54: 10, 56: 10, 58: 3, 60: 3})
    p, _, _ = vgs.parse_task_file(str(f))
    assert p.method == 3 and p.adjacency_min == 3
    np.testing.assert_array_equal(np.float32([p.voxel_size, p.seed_size, p.graph_size, p.sig_w, p.cut_thred, p.color_impt, p.spatial_impt, p.normal_impt]),
                                  np.float32([0.05, 0.25, 0.5, 1, 0.5, 0, 0.25, 0.75]))


def test_parse_reference_task_files_if_present(vgs):
    """The stock task files (tests/golden/task_*_stock.txt: the reference's line layout and parameter values) parse to the defaults."""
    golden = os.path.join(ROOT, "tests", "golden")
    p, inn, out = vgs.parse_task_file(os.path.join(golden, "task_vgs_stock.txt"))
    d = vgs.default_params(2)
    assert (inn, out) == ("Town_Test.pcd", "Town_Test_VGS.pcd")
    for k in ("voxel_size", "graph_size", "sig_p", "sig_n", "sig_o", "sig_e", "sig_c", "sig_w", "cut_thred", "points_min", "adjacency_min", "voxels_min"):
        assert getattr(p, k) == getattr(d, k), k
    p3, _, _ = vgs.parse_task_file(os.path.join(golden, "task_svgs_stock.txt"))
    d3 = vgs.default_params(3)
    for k in ("voxel_size", "seed_size", "graph_size", "sig_w", "cut_thred", "color_impt", "spatial_impt", "normal_impt", "adjacency_min"):
        assert getattr(p3, k) == getattr(d3, k), k


def test_no_cpu_fallback(vgs):
    """Without a HIP device the engine refuses to exist (the driver runs this file on a GPU-less container)."""
    import conftest
    if conftest._has_gpu():
        pytest.skip("GPU present")
    with pytest.raises(vgs.VgsError) as e:
        vgs.Engine(vgs.default_params(2))
    assert e.value.status == vgs._lib.VGS_E_HIP


def test_scenes_are_deterministic(vgs):
    a = vgs.scenes.urban_scene(5000)
    b = vgs.scenes.urban_scene(5000)
    assert a.dtype == np.float32 and a.shape == (5000, 3)
    np.testing.assert_array_equal(a, b)
    assert np.abs(a).max() < 150 and (a != 0).all()
    t0 = vgs.scenes.tiled_urban_scene(16000, tiles=(2, 1), tile_index=0)
    t1 = vgs.scenes.tiled_urban_scene(16000, tiles=(2, 1), tile_index=1)
    both = vgs.scenes.tiled_urban_scene(16000, tiles=(2, 1))
    np.testing.assert_array_equal(np.concatenate([t0, t1]), both)
    assert t0[:, 0].mean() < 0 < t1[:, 0].mean()


def test_schedule_bounds_dominate_weight(oracle):
    """csrc/vgs_math.h: vm_weight_bound_da >= weight and vm_weight_bound_d >= weight for every pair -- the two
    facts the lazy local cut's evaluation order relies on."""
    rng = np.random.default_rng(11)
    for svgs, P in ((False, oracle.vgs_params(math=1)), (True, oracle.svgs_params(math=1)), (False, oracle.vgs_params(math=1, sig_p=0.05, sig_n=1.5, sig_w=0.7))):
        for _ in range(4000):
            def node():
                c = rng.standard_normal(3) * rng.choice([0.05, 0.3, 2.0]) + np.array([3.0, -2.0, 1.0])
                n = rng.standard_normal(3)
                n /= np.linalg.norm(n)
                f = rng.random(8)
                nd = oracle.node16(c, n, f)
                if rng.random() < 0.03:
                    nd[rng.integers(0, 3)] = 0.0      # invalid position
                if rng.random() < 0.03:
                    nd[3 + rng.integers(0, 3)] = 0.0  # invalid normal
                return nd
            a, b = node(), node()
            if rng.random() < 0.3:
                b[3:6] = a[3:6] + rng.standard_normal(3).astype(np.float32) * 1e-3   # nearly parallel normals
                b[3:6] /= np.linalg.norm(b[3:6])
            w, ub_da, ub_d = oracle.weight_and_bounds(a, b, P, svgs)
            if np.isnan(w):
                continue
            assert np.isnan(ub_da) or ub_da >= w, (w, ub_da)
            assert ub_d >= w, (w, ub_d)


def test_screen_table_never_drops_a_heavy_pair(vgs, oracle):
    """The dense hand-over kernels (csrc/localcut_dense.hpp) do not evaluate a pair whose centroid distance reaches d2_stop or
    whose normals' dot product is at or below the table's cosine for its distance bin.  Whatever they drop must weigh at most
    1 - cut: the table (vgs_screen_table, host arithmetic of csrc/localcut.hip) against the DevMath weight of random pairs,
    with the kernel's float expressions restated in numpy."""
    import ctypes as C
    f32 = np.float32
    L = vgs._lib.lib()
    rng = np.random.default_rng(23)
    sets = [(False, vgs.default_params(2), oracle.vgs_params(math=1)),
            (False, vgs.default_params(2, voxel_size=0.05, cut_thred=0.6, sig_n=0.5), oracle.vgs_params(math=1, voxel_size=0.05, cut_thred=0.6, sig_n=0.5)),
            (False, vgs.default_params(2, sig_p=0.05, sig_w=0.7, cut_thred=0.1), oracle.vgs_params(math=1, sig_p=0.05, sig_w=0.7, cut_thred=0.1)),
            (True, vgs.default_params(3), oracle.svgs_params(math=1))]
    for svgs, p, P in sets:
        d2_stop, scale = C.c_float(), C.c_float()
        tab = np.zeros(64, dtype=np.float32)
        assert L.vgs_screen_table(C.byref(p), C.byref(d2_stop), C.byref(scale), tab.ctypes.data_as(C.c_void_p)) == 0
        d2_stop, scale = f32(d2_stop.value), f32(scale.value)
        thr0 = f32(1.0) - f32(p.cut_thred) / f32(1.0)
        valid = tab[tab > -2.0]
        assert (valid[:-1] <= valid[1:]).all() and (valid <= 1.0).all()      # farther apart, smaller angles suffice
        dropped = kept = 0
        reach = np.sqrt(min(float(d2_stop), 4.0)) if np.isfinite(d2_stop) else 1.5
        for _ in range(6000):
            c1 = (rng.standard_normal(3) * 0.5 + np.array([3.0, -2.0, 1.0])).astype(np.float32)
            c2 = (c1 + rng.standard_normal(3) * reach * rng.choice([0.1, 0.5, 1.0])).astype(np.float32)
            n1 = rng.standard_normal(3); n1 /= np.linalg.norm(n1)
            n2 = n1 + rng.standard_normal(3) * rng.choice([1e-3, 0.05, 0.3, 2.0]); n2 /= np.linalg.norm(n2)
            a, b = oracle.node16(c1, n1, rng.random(8)), oracle.node16(c2, n2, rng.random(8))
            if rng.random() < 0.05:
                b[3:6] = a[3:6]                                            # identical normals: dot may round above 1
            w, ub_da, _ = oracle.weight_and_bounds(a, b, P, svgs)
            d = a[0:3] - b[0:3]
            d2 = f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])
            pos = bool((a[0:3] != 0).all() and (b[0:3] != 0).all())
            nrm = bool((a[3:6] != 0).all() and (b[3:6] != 0).all())
            if pos and d2 >= d2_stop:
                drop = True
            elif pos and nrm and d2 > 0:
                k = min(63, int(f32(d2 * scale)))
                dot = f32(f32(a[3] * b[3]) + f32(a[4] * b[4])) + f32(a[5] * b[5])
                drop = bool(dot <= tab[k] and dot >= f32(-1.0))
            else:
                drop = bool(ub_da <= thr0)
            if drop:
                dropped += 1
                assert not (w > thr0), (svgs, w, thr0, d2, ub_da)
            else:
                kept += 1
        # at the table's edge: pairs whose dot product straddles the cosine of their bin by a few ulps -- a dropped pair's
        # float bound (vm_weight_bound_da, which dominates the weight) must already be at or below the threshold
        for _ in range(3000 if len(valid) else 0):
            k = int(rng.integers(0, 64))
            if tab[k] <= -2.0:
                continue
            dist = np.sqrt((k + rng.random()) / float(scale))
            u = rng.standard_normal(3); u /= np.linalg.norm(u)
            c1 = np.array([3.0, -2.0, 1.0]) + rng.standard_normal(3) * 0.3
            n1 = rng.standard_normal(3); n1 /= np.linalg.norm(n1)
            t = np.cross(n1, rng.standard_normal(3)); t /= np.linalg.norm(t)
            ang = np.arccos(np.clip(float(tab[k]), -1, 1)) + rng.choice([-3e-6, -1e-6, -3e-7, 0.0, 3e-7, 1e-6, 3e-6])
            n2 = np.cos(ang) * n1 + np.sin(ang) * t
            a, b = oracle.node16(c1, n1, rng.random(8)), oracle.node16(c1 + dist * u, n2, rng.random(8))
            w, ub_da, _ = oracle.weight_and_bounds(a, b, P, svgs)
            d = a[0:3] - b[0:3]
            d2 = f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])
            if d2 >= d2_stop or not d2 > 0:
                continue
            kk = min(63, int(f32(d2 * scale)))
            dot = f32(f32(a[3] * b[3]) + f32(a[4] * b[4])) + f32(a[5] * b[5])
            if dot <= tab[kk] and dot >= f32(-1.0):
                assert ub_da <= thr0 and not (w > thr0), (svgs, kk, dot, tab[kk], ub_da, thr0, w)
        assert kept > 300 and (dropped > 500 or len(valid) == 0), (dropped, kept)     # the sample exercises both sides (a loose cut
        # with wide sigmas has no table: nothing can be proved from distance and angle alone)


def _pcl_grow(state, pts, res):
    """PCL OctreePointCloud::adoptBoundingBoxToPoint over pts in order, as k_adopt / OctreeBox::adopt do it.
    state = (min[3], shift[3], depth) of a defined box; returns the new state."""
    eps = 1.1920928955078125e-07
    mn, sh, depth = [float(v) for v in state[0]], [int(v) for v in state[1]], int(state[2])
    for p in pts:
        while True:
            side = float(1 << depth) * res
            mx = [mn[a] + side - eps for a in range(3)]
            hi = [float(p[a]) >= mx[a] for a in range(3)]
            if not any(hi[a] or float(p[a]) < mn[a] for a in range(3)):
                break
            for a in range(3):
                if not hi[a]:
                    mn[a] -= side
                    sh[a] += 1 << depth
            depth += 1
    return mn, sh, depth


def test_grid_replay_from_bounding_boxes(vgs):
    """vgs_grid_advance_bbox (host arithmetic of the tile chain): wherever it advances the grid from a cloud's bounding box
    alone, the state equals PCL's growth over the points themselves; wherever it asks for a scan, continuing with the
    points from the state it reached ends where the growth over the points from the start ends."""
    import ctypes as C
    from vgs_svgs_segmentation_amd._lib import VgsGridState, lib
    L = lib()
    rng = np.random.default_rng(3)
    res = float(np.float32(0.1))
    n_direct = n_scan = 0
    for trial in range(300):
        depth = int(rng.integers(3, 9))
        side = (1 << depth) * res
        mn = (rng.random(3) * 20.0 - 10.0)
        start = (mn.tolist(), [int(x) for x in rng.integers(0, 1000, 3)], depth)
        # a tile somewhere around the box: inside, beside on one axis, on a diagonal, below ...
        centre = mn + side * (0.5 + rng.integers(-2, 3, 3) * rng.random(3) * 1.5)
        ext = side * (0.05 + rng.random(3))
        pts = (centre + (rng.random((200, 3)) - 0.5) * ext).astype(np.float32)
        g = VgsGridState()
        L.vgs_grid_state_init(C.byref(g))
        for a in range(3):
            g.min[a] = start[0][a]
            g.shift[a] = start[1][a]
        g.depth, g.defined = depth, 1
        bb = np.concatenate([pts.min(0), pts.max(0)]).astype(np.float32)
        need = C.c_int32(0)
        assert L.vgs_grid_advance_bbox(C.byref(g), C.c_double(res), bb.ctypes.data_as(C.c_void_p), C.byref(need)) == 0
        want = _pcl_grow(start, pts, res)
        reached = ([g.min[a] for a in range(3)], [int(g.shift[a]) for a in range(3)], int(g.depth))
        if need.value:
            n_scan += 1
            reached = _pcl_grow(reached, pts, res)
        else:
            n_direct += 1
        assert reached[2] == want[2] and reached[1] == want[1] and reached[0] == want[0], (trial, need.value, reached, want)
    assert n_direct > 50 and n_scan > 20, (n_direct, n_scan)
    # an undefined grid always needs the points: its first box is placed around the first point
    g = VgsGridState()
    L.vgs_grid_state_init(C.byref(g))
    need = C.c_int32(0)
    assert L.vgs_grid_advance_bbox(C.byref(g), C.c_double(res), np.zeros(6, np.float32).ctypes.data_as(C.c_void_p), C.byref(need)) == 0 and need.value == 1


def test_p2_protocol_catches_what_it_is_for():
    """tests/helpers.p2_protocol: identical partitions pass under renaming; a big segment split in two fails the
    IoU clause although 99.5 % agreement alone would not notice a small scene's; dropped small segments fail the count clause."""
    from helpers import assert_p2, p2_protocol
    rng = np.random.default_rng(1)
    V = 4000
    pv = np.repeat(np.arange(V), 5)                       # five points per voxel
    seg = np.minimum(np.arange(V) // 40, 60)              # 60 segments of 40 voxels and a large one
    ref = seg[pv]
    perm = rng.permutation(seg.max() + 1)
    r = assert_p2(perm[seg][pv], ref, pv)                 # renaming does not matter
    assert r["agreement"] == 1.0 and r["min_iou"] == 1.0 and r["big_segments"] == 61 and r["kept_ref"] == 61
    split = seg.copy()
    split[:3] = 99                                        # three voxels of a 40-voxel segment elsewhere: IoU 37/40
    r = p2_protocol(split[pv], ref, pv)
    assert r["agreement"] > 0.999 and abs(r["min_iou"] - 37 / 40) < 1e-9 and r["worst"]["ref_label"] == 0
    with pytest.raises(AssertionError):
        assert_p2(split[pv], ref, pv)
    merged = np.where(seg == 1, 0, seg)                   # two oracle segments under one label: IoU 0.5 for both
    with pytest.raises(AssertionError):
        assert_p2(merged[pv], ref, pv)
    dropped = np.where(seg < 2, -1, seg)                  # two of 61 segments dropped: count off by 3 %
    r = p2_protocol(dropped[pv], ref, pv)
    assert r["kept_test"] == 59 and r["min_iou"] == 0.0
    used = np.ones(V, bool)
    used[:80] = False                                     # agreement is over USED voxels only
    assert p2_protocol(dropped[pv], ref, pv, used)["agreement"] == 1.0
