"""Connected parts of a caller's per-POINT labelling on the device (vgs_point_label_components, csrc/labelcc.hip; Engine.label_components)
against tests/label_components_ref.py, the numpy restatement of the definition in include/vgs.h, fed the engine's own point_voxel() and
lists(0) -- every table compared with `==`, no tolerance:
  * the engine's own labels; the bridge through unused voxels that an implementation reading only the stored rows misses; the reach of
    graph_size between two slabs; labels that alternate inside nodes; a serpentine of 4 000 voxels (depth of the union-find); many tiny
    parts, one giant part and runs of empty labels (contention and lookup); rows above 64 and above 1 024 entries; the edge inputs; SVGS;
  * composition with describe_labels; the refined labels; determinism and input forms; the status contract."""
import ctypes as C

import numpy as np
import pytest

import label_components_ref as R
from label_refine_ref import floor_and_wall
from label_refine_scenes import GROUP5, SPLIT, WALL, _voxel_points, big_boundary_voxel, blob, dropped_beside_kept, grid_supervoxels, mirror_pair
from segment_scenes import two_tilted_planes

pytestmark = pytest.mark.gpu

LC_SHORT = 64   # rows up to so many entries share a wavefront (csrc/labelcc.hip)


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


def _graph(eng):
    """what the restatement reads besides the labels: the node of every point and the rows of every node"""
    return (eng.point_voxel(),) + tuple(eng.lists("adjacency"))


def _check(eng, graph, labels, K):
    """label_components on the engine and by the restatement: equal tables and counts; returns the engine's"""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    got = eng.label_components(labels, K)
    ref = R.label_components(labels, graph[0], graph[1], graph[2], K)
    print(K, got["n_parts"], got["n_skipped"])
    assert not R.same(got, ref), (R.same(got, ref), got["n_parts"], ref["n_parts"])
    return got


# ---------------------------------------------------------------- the engine's own labels
@pytest.mark.parametrize("name", ["planes", "dropped"])
def test_own_point_labels(gpu, name):
    xyz = two_tilted_planes() if name == "planes" else dropped_beside_kept()
    eng = _vgs(gpu, xyz, **GROUP5)
    labels, K = eng.point_labels(), eng.counts()["kept"]
    assert K >= 1 and (labels >= 0).any()
    got = _check(eng, _graph(eng), labels, K)
    assert eng.label_components(labels)["part_of_point"].tobytes() == got["part_of_point"].tobytes()   # K None: max + 1 = kept
    # a kept segment is connected through mutual connections, which are adjacency entries: every label is one part
    assert (np.diff(got["label_first"]) == 1).all()
    assert np.array_equal(got["part_of_point"], labels)
    assert np.array_equal(got["label_first"], np.arange(K + 1))
    assert np.array_equal(got["label_largest"], np.arange(K)) and np.array_equal(got["part_label"], np.arange(K))
    if name == "planes":
        assert K >= 2


# ---------------------------------------------------------------- the bridge through unused voxels
def test_bridge_through_unused_voxels(gpu):
    xyz = dropped_beside_kept()
    eng = _vgs(gpu, xyz, **GROUP5)
    graph = _graph(eng)
    finite = np.isfinite(xyz).all(axis=1)
    labels = np.zeros(xyz.shape[0], np.int32)   # the NaN and infinite points carry the label too: skipped
    labels[0] = -1   # (the first point, on a voxel corner, sits in a voxel of its own two diagonal steps from the kept row)
    got = _check(eng, graph, labels, 1)
    pv, used = graph[0], eng.attributes()["used"]
    assert (pv[~finite] == -1).all() and got["n_skipped"] == int((~finite).sum()) == 4 and (got["part_of_point"][~finite] == -1).all()
    pop = got["part_of_point"]

    def part_of_voxel(ijk):
        m = np.all(np.floor(xyz[finite] / np.float32(0.1)).astype(int) == np.asarray(ijk), axis=1)
        p = np.unique(pop[finite][m])
        assert m.sum() > 0 and p.size == 1, (ijk, m.sum(), p)
        return int(p[0]), np.unique(pv[finite][m])

    kept = [part_of_voxel((2 + i, 2, 2)) for i in range(4)]
    bridge = [part_of_voxel((2, 2, 3)), part_of_voxel((2, 2, 4))]
    dropped = [part_of_voxel((2 + i, 2, 5)) for i in range(2)]
    lone = part_of_voxel((40, 2, 2))
    assert all(used[v].all() for _, v in kept + dropped) and not any(used[v].any() for _, v in bridge + [lone])
    assert {p for p, _ in kept + bridge + dropped} == {kept[0][0]} and lone[0] != kept[0][0]
    assert got["n_parts"] == 2 and got["part_label"].tolist() == [0, 0] and got["label_first"].tolist() == [0, 2]
    assert got["label_largest"].tolist() == [kept[0][0]]


# ---------------------------------------------------------------- reach
@pytest.mark.parametrize("shift,parts", [((3, 0, 0), 2), ((2, 0, 0), 1), ((2, 4, 0), 2), ((2, 3, 1), 1)],
                         ids=["two_steps", "one_step", "diagonal_above", "diagonal_below"])
def test_reach_between_two_slabs(gpu, shift, parts):
    """Slabs of 3 x 3 voxels in the y-z plane.  Two empty steps along x: centre distance 0.3; one: 0.2; the nearest pair offset by
    (2, 2, 0): 0.283, the smallest lattice distance above 0.25; by (2, 1, 1): 0.245, the largest below."""
    rng = np.random.default_rng(21)
    a = [(2, 2 + j, 2 + k) for j in range(3) for k in range(3)]
    b = [(2 + shift[0], 2 + j + shift[1], 2 + k + shift[2]) for j in range(3) for k in range(3)]
    if shift == (2, 3, 1):   # one voxel of the second slab only, so that the nearest pair is (2, 1, 1) apart
        b = [(4, 5, 5)]
    xyz = np.concatenate([np.array([[0.1, 0.1, 0.1]])] + [_voxel_points(rng, v, 8) for v in a + b]).astype(np.float32)
    eng = _vgs(gpu, xyz, **GROUP5)
    assert eng.params.graph_size == np.float32(0.25) and eng.params.voxel_size == np.float32(0.1)
    labels = np.zeros(xyz.shape[0], np.int32)
    labels[0] = -1
    got = _check(eng, _graph(eng), labels, 1)
    assert got["n_parts"] == parts and got["part_nodes"].sum() == len(a) + len(b) and got["part_of_point"][0] == -1


# ---------------------------------------------------------------- labels that alternate inside nodes
def test_labels_alternate_inside_nodes(gpu):
    xyz = big_boundary_voxel()
    eng = _vgs(gpu, xyz, **SPLIT)
    graph = _graph(eng)
    assert np.bincount(graph[0][graph[0] >= 0]).max() >= 5000
    labels = (np.arange(xyz.shape[0]) % 3).astype(np.int32)
    got = _check(eng, graph, labels, 3)
    assert got["part_nodes"].sum() > eng.counts()["voxels"]   # several vertices per node
    _check(eng, graph, labels, 7)   # and with empty labels behind


# ---------------------------------------------------------------- depth
def _serpentine(rows=62, length=64):
    """a one-voxel-wide path in the plane z = 2: rows of `length` voxels along x, two lattice steps apart in y, joined at alternating
    ends by one voxel; in path order"""
    path = []
    for r in range(rows):
        xs = range(length) if r % 2 == 0 else range(length - 1, -1, -1)
        path += [(2 + x, 2 + 2 * r, 2) for x in xs]
        if r + 1 < rows:
            path.append((path[-1][0], 3 + 2 * r, 2))
    return path


def test_serpentine_of_4000_voxels(gpu):
    params = dict(GROUP5, graph_size=0.18)   # the 26 neighbours only: sqrt(3) * 0.1 < 0.18 < 0.2
    path = _serpentine()
    per = params["points_min"] + 1
    rng = np.random.default_rng(4)
    xyz = np.concatenate([np.array([[0.1, 0.1, 0.1]])] + [_voxel_points(rng, v, per) for v in path]).astype(np.float32)
    eng = _vgs(gpu, xyz, **params)
    graph = _graph(eng)
    assert len(path) >= 4000 and np.unique(graph[0][1:]).size == len(path)
    labels = np.zeros(xyz.shape[0], np.int32)
    labels[0] = -1
    got = _check(eng, graph, labels, 1)
    assert got["n_parts"] == 1 and got["part_nodes"].tolist() == [len(path)] and got["part_points"].tolist() == [per * len(path)]
    # every 500th voxel of the path relabelled
    step = np.arange(len(path)) % 500 == 0
    labels[1:] = np.repeat(step.astype(np.int32), per)
    got = _check(eng, graph, labels, 2)
    assert got["n_parts"] > 2 and got["label_first"][1] >= 2


# ---------------------------------------------------------------- contention and lookup
_cube = {}


def _cube_scene(gpu):
    if not _cube:
        xyz = np.random.default_rng(8).uniform(0.0, 2.0, size=(20_000, 3)).astype(np.float32)
        eng = _vgs(gpu, xyz, **GROUP5)
        _cube.update(xyz=xyz, eng=eng, graph=_graph(eng))
    return _cube["xyz"], _cube["eng"], _cube["graph"]


@pytest.mark.parametrize("kind", ["many_tiny", "one_giant", "sparse_k"])
def test_contention_and_lookup(gpu, kind):
    xyz, eng, graph = _cube_scene(gpu)
    n = xyz.shape[0]
    rng = np.random.default_rng(9)
    if kind == "many_tiny":
        labels, K = rng.integers(0, 1000, size=n).astype(np.int32), 1000
    elif kind == "one_giant":
        labels, K = np.zeros(n, np.int32), 1
    else:
        labels, K = (rng.integers(0, 5, size=n) * 9973 + 17).astype(np.int32), 50_000
    got = _check(eng, graph, labels, K)
    used = eng.attributes()["used"]
    assert used.any() and not used.all()   # stored rows and rows built on request
    if kind == "many_tiny":
        assert got["n_parts"] > 5000 and got["part_nodes"].sum() > eng.counts()["voxels"]
    elif kind == "one_giant":
        assert got["part_points"].max() > n // 2
    else:
        assert (np.diff(got["label_first"]) == 0).sum() == K - 5 and (got["label_largest"] >= 0).sum() == 5


# ---------------------------------------------------------------- long rows
def test_rows_above_64_and_above_1024_entries(gpu):
    xyz = np.random.default_rng(12).uniform(0.0, 1.3, size=(12_000, 3)).astype(np.float32)
    eng = _vgs(gpu, xyz, voxel_size=0.1, graph_size=0.7, points_min=3, voxels_min=0)
    counts = eng.adjacency_counts()
    graph = _graph(eng)
    rows = np.diff(graph[1])
    used = eng.attributes()["used"] != 0
    assert counts.max() > 1024 and ((counts > LC_SHORT) & (counts <= 1024)).any()
    assert used.any() and (~used).any() and rows[~used].max() > 1024   # the rows built on request are long too
    labels = np.where(xyz[:, 0] < 0.8, 0, 1).astype(np.int32)
    labels[::7] = -1
    got = _check(eng, graph, labels, 2)
    assert got["n_parts"] >= 2


# ---------------------------------------------------------------- edge inputs
def test_edge_inputs(gpu):
    xyz = dropped_beside_kept()
    eng = _vgs(gpu, xyz, **GROUP5)
    graph = _graph(eng)
    n = xyz.shape[0]
    assert _check(eng, graph, np.zeros(n, np.int32), 1)["n_parts"] == 3   # the kept row and its bridge, the lone voxel, the first point's voxel
    for labels, K in ((np.full(n, -1, np.int32), 0), (np.full(n, -1, np.int32), 3), (np.full(n, -7, np.int32), 1)):
        got = _check(eng, graph, labels, K)
        assert got["n_parts"] == 0 and (got["part_of_point"] == -1).all() and got["part_label"].size == 0
        assert got["label_first"].tolist() == [0] * (K + 1) and got["label_largest"].tolist() == [-1] * K
    # labels only on points outside the octree
    finite = np.isfinite(xyz).all(axis=1)
    got = _check(eng, graph, np.where(finite, -1, 2).astype(np.int32), 3)
    assert got["n_parts"] == 0 and got["n_skipped"] == int((~finite).sum()) and (got["part_of_point"] == -1).all()
    assert eng.label_components(np.full(n, -1, np.int32))["label_first"].tolist() == [0]   # K None of an all-negative labelling: 0


@pytest.mark.parametrize("kind", ["no_finite_point", "empty_cloud"])
def test_clouds_without_a_node(gpu, kind):
    xyz = np.full((5, 3), np.nan, np.float32) if kind == "no_finite_point" else np.zeros((0, 3), np.float32)
    eng = _vgs(gpu, xyz, **GROUP5)
    n = xyz.shape[0]
    got = eng.label_components(np.zeros(n, np.int32), 2)
    assert got["n_parts"] == 0 and got["n_skipped"] == n and got["part_of_point"].tolist() == [-1] * n
    assert got["label_first"].tolist() == [0, 0, 0] and got["label_largest"].tolist() == [-1, -1]
    assert all(got[f].size == 0 for f in ("part_label", "part_points", "part_nodes", "part_first_node"))


# ---------------------------------------------------------------- SVGS
def test_svgs_mirror_pair_and_grid_supervoxels(gpu):
    xyz, sv, mx = mirror_pair()
    eng = _svgs(gpu, xyz, sv, mx)
    graph = _graph(eng)
    n = xyz.shape[0]
    _check(eng, graph, np.zeros(n, np.int32), 1)
    _check(eng, graph, (np.arange(n) % 2).astype(np.int32), 2)
    _check(eng, graph, eng.point_labels(), eng.counts()["kept"])
    xyz = blob(n=6000)
    sv, mx = grid_supervoxels(xyz)
    eng = _svgs(gpu, xyz, sv, mx)
    graph = _graph(eng)
    got = _check(eng, graph, (xyz[:, 0] > 0).astype(np.int32) + (xyz[:, 1] > 0.4), 3)
    assert got["part_nodes"].sum() > eng.counts()["voxels"]
    _check(eng, graph, eng.point_labels(), eng.counts()["kept"])


# ---------------------------------------------------------------- composition with the other tables of a labelling
def test_composition_with_describe_labels(gpu):
    xyz, eng, graph = _cube_scene(gpu)
    labels = (np.random.default_rng(2).integers(-1, 40, size=xyz.shape[0])).astype(np.int32)
    K = 40
    got = eng.label_components(labels, K)
    C_ = got["n_parts"]
    assert C_ > K
    d = eng.describe_labels(got["part_of_point"], K=C_)
    assert np.array_equal(d["n_points"], got["part_points"]) and np.array_equal(d["n_nodes"], got["part_nodes"])
    whole = eng.describe_labels(labels, K=K)
    lf = got["label_first"]
    sums = np.array([got["part_points"][lf[k]:lf[k + 1]].sum() for k in range(K)], np.int64)
    assert np.array_equal(sums, whole["n_points"]) and got["n_skipped"] == whole["n_skipped"]
    assert np.array_equal(np.diff(lf) > 0, whole["n_points"] > 0)


# ---------------------------------------------------------------- the refined labels
def test_parts_of_the_refined_labels(gpu):
    xyz = floor_and_wall()[0]
    eng = _vgs(gpu, xyz, **WALL)
    eng.refine_labels()
    refined, K = eng.refined_labels(), eng.counts()["kept"]
    graph = _graph(eng)
    got = _check(eng, graph, refined, K)
    assert got["n_parts"] >= K >= 2
    assert np.array_equal(eng.refined_labels(), refined)   # the refinement's own buffer is untouched


# ---------------------------------------------------------------- determinism and input forms
def test_determinism_and_input_forms(gpu):
    torch = pytest.importorskip("torch")
    xyz, eng, graph = _cube_scene(gpu)
    n = xyz.shape[0]
    labels = np.random.default_rng(3).integers(-1, 30, size=n).astype(np.int32)
    a = eng.label_components(labels, 30)
    assert not R.same(eng.label_components(labels, 30), a)
    other = _vgs(gpu, xyz, **GROUP5)
    assert not R.same(other.label_components(labels, 30), a)
    dev = torch.from_numpy(labels).to("cuda:0")
    assert not R.same(eng.label_components(dev, 30), a)
    assert not R.same(eng.label_components(dev), a)   # K None on the device: max + 1
    # other table calls in between leave the result where it is
    ptrs = eng.label_components_device()
    eng.describe_labels(labels, K=30)
    eng.label_boxes(labels, K=30)
    eng.compare_labels((labels % 5).astype(np.int32), labels=labels, K=30)
    eng.refine_labels()
    eng.segment_descriptors()
    out = {name: np.zeros(a[name].shape, a[name].dtype) for name, _, _ in gpu.Engine.COMPONENT_FIELDS}
    eng._ck(eng._L.vgs_get_point_label_components(eng._h, *(out[name].ctypes.data_as(C.c_void_p) for name, _, _ in gpu.Engine.COMPONENT_FIELDS)))
    assert all(out[name].tobytes() == a[name].tobytes() for name in out)
    assert eng.label_components_device() == ptrs and all(v for v in ptrs.values())
    part = torch.zeros(a["n_parts"], dtype=torch.int64, device="cuda:0")
    C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(C.c_void_p(part.data_ptr()), C.c_void_p(ptrs["part_points"]), C.c_size_t(8 * a["n_parts"]), 3)
    assert np.array_equal(part.cpu().numpy(), a["part_points"])
    # any pointer may be NULL
    eng._ck(eng._L.vgs_get_point_label_components(eng._h, *([None] * 7)))


# ---------------------------------------------------------------- the status contract
def test_status_contract(gpu):
    lib = gpu._lib
    xyz = dropped_beside_kept()
    n = xyz.shape[0]
    labels = np.zeros(n, np.int32)
    eng = gpu.Engine(gpu.default_params(2, **GROUP5))
    eng.set_points(xyz)
    with pytest.raises(gpu.VgsError) as e:   # before a run
        eng.label_components(labels, 1)
    assert e.value.status == lib.VGS_E_STATE
    eng.run()
    with pytest.raises(gpu.VgsError) as e:   # a getter before a compute call
        eng.label_components_device()
    assert e.value.status == lib.VGS_E_STATE
    with pytest.raises(gpu.VgsError) as e:
        eng._ck(eng._L.vgs_get_point_label_components(eng._h, *([None] * 7)))
    assert e.value.status == lib.VGS_E_STATE
    with pytest.raises(gpu.VgsError) as e:   # n != N
        eng.label_components(labels[:-1], 1)
    assert e.value.status == lib.VGS_E_ARG
    bad = labels.copy()
    bad[7], bad[11] = 3, 9
    with pytest.raises(gpu.VgsError) as e:   # a label >= K: the error and the index of describe_labels
        eng.label_components(bad, 3)
    with pytest.raises(gpu.VgsError) as d:
        eng.describe_labels(bad, K=3)
    assert e.value.status == d.value.status == lib.VGS_E_ARG and "labels[7] = 3" in str(e.value)
    assert str(e.value).split(": ", 2)[2] == str(d.value).split(": ", 2)[2]
    with pytest.raises(gpu.VgsError) as e:   # ... and it left no result behind
        eng.label_components_device()
    assert e.value.status == lib.VGS_E_STATE
    assert eng.label_components(labels, 1)["n_parts"] == 3
    eng.label_components_device()
    eng.run()   # a new run of the stages
    with pytest.raises(gpu.VgsError) as e:
        eng.label_components_device()
    assert e.value.status == lib.VGS_E_STATE
    # a tile context is refused, the limitation named
    t = gpu.Engine(gpu.default_params(2, **GROUP5))
    t.set_points(xyz)
    lo, hi = np.array([-1e9, -1e9], dtype=np.float64), np.array([1e9, 1e9], dtype=np.float64)
    t._ck(t._L.vgs_set_owned_region(t._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    t.run()
    with pytest.raises(gpu.VgsError) as e:
        t.label_components(labels, 1)
    assert e.value.status == lib.VGS_E_STATE and "tile context" in str(e.value) and "across the ranks" in str(e.value)
