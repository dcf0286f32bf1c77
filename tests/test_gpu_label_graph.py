"""Adjacency graph of a caller's per-POINT labelling on the device (vgs_point_label_graph, csrc/labelgraph.hip; Engine.label_graph) against
tests/label_graph_ref.py, the numpy restatement of the definition in include/vgs.h, fed the engine's own point_voxel(), lists(0), used
flags and local-cut weights (helpers.pair_weights).  Integer fields, seg_ab, w_min and w_max are compared with `==` (the floats as bit
patterns), w_sum is held to helpers.check_graph's bar |got - ref| <= 1e-10 |ref|; the weights of every edge are checked."""
import ctypes as C

import numpy as np
import pytest

import helpers
import label_graph_ref as R
from label_refine_ref import floor_and_wall
from label_refine_scenes import GROUP5, SPLIT, WALL, _voxel_points, big_boundary_voxel, blob, dropped_beside_kept, grid_supervoxels, mirror_pair
from segment_scenes import two_tilted_planes

pytestmark = pytest.mark.gpu

LG_CHUNK = 256   # records per chunk of an edge's fold (csrc/labelgraph.hip)
# GROUP5's nodes (voxels of at most five points unused) under the default cut: unused voxels are inert, the stored rows pruned to used neighbours
PRUNED5 = dict(voxel_size=0.1, graph_size=0.25, points_min=5, voxels_min=2)


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


def _inputs(eng):
    """what the restatement reads besides the labels: the node of every point, the rows of every node, the used flags"""
    return (eng.point_voxel(),) + tuple(eng.lists("adjacency")) + (eng.attributes()["used"].astype(bool),)


def _ref(eng, inp, labels, K):
    return R.label_graph(labels, inp[0], inp[1], inp[2], inp[3], K, lambda a, b: helpers.pair_weights(eng, a, b))


def _check(eng, inp, labels, K):
    """label_graph on the engine and by the restatement: equal tables; returns the engine's"""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    got = eng.label_graph(labels, K)
    ref = _ref(eng, inp, labels, K)
    print(K, got["n_edges"], ref["n_edges"], got["n_skipped"], got["n_pairs"][:8], ref["n_pairs"][:8], got["w_sum"][:4], ref["w_sum"][:4])
    assert R.diff(got, ref) == [], R.diff(got, ref)
    a, b = got["seg_ab"][:, 0].astype(np.int64), got["seg_ab"][:, 1].astype(np.int64)
    assert (a < b).all() and (a >= 0).all() and (b < max(K, 1)).all() and (np.diff(a * (1 << 32) + b) > 0).all()
    assert (got["n_finite"] <= got["n_pairs"]).all() and ((got["n_pairs"] > 0) | (got["n_shared"] > 0)).all()
    return got


def _stored_rows_hold_unused(eng, inp):
    """Which once-per-contact branch the engine takes, read from its results: vgs_get_lists(0) names every neighbour of every node whatever
    the engine stores, vgs_get_local_weights reports a used node's STORED row, which is pruned to used neighbours when unused voxels are
    inert."""
    _, off, idx, used = inp
    has_unused = np.add.reduceat((~used[idx]).astype(np.int64), off[:-1]) > 0
    v = int(np.nonzero(used & has_unused)[0][0])
    ids, _ = eng.local_weights(v)
    return bool((~used[ids]).any())


def _voxel_of(xyz, ijk, voxel=0.1):
    with np.errstate(invalid="ignore"):
        return np.all(np.floor(xyz / np.float32(voxel)) == np.asarray(ijk, dtype=np.float32), axis=1)


# ---------------------------------------------------------------- the engine's own labels
@pytest.mark.parametrize("name", ["planes", "dropped", "wall"])
def test_own_point_labels_give_the_segment_graph(gpu, name):
    """(under GROUP5 the two planes are two segments out of each other's reach and the dropped scene keeps one: no edge in either graph;
    floor and wall under WALL touch)"""
    xyz = {"planes": two_tilted_planes, "dropped": dropped_beside_kept, "wall": lambda: floor_and_wall()[0]}[name]()
    eng = _vgs(gpu, xyz, **(WALL if name == "wall" else GROUP5))
    labels, K = eng.point_labels(), eng.counts()["kept"]
    got = _check(eng, _inputs(eng), labels, K)
    seg = eng.segment_graph()
    assert (got["n_shared"] == 0).all()
    for k in ("seg_ab", "n_pairs", "n_finite", "nodes_ab"):
        assert np.array_equal(got[k], seg[k]), k
    assert got["w_min"].tobytes() == seg["w_min"].tobytes() and got["w_max"].tobytes() == seg["w_max"].tobytes()
    assert (np.abs(got["w_sum"] - seg["w_sum"]) <= 1e-10 * np.abs(seg["w_sum"])).all()
    print("w_sum byte-equal to segment_graph():", got["w_sum"].tobytes() == seg["w_sum"].tobytes(), got["n_edges"])
    assert eng.label_graph(labels)["seg_ab"].tobytes() == got["seg_ab"].tobytes()   # K None: max + 1
    helpers.check_graph(eng)   # and the segment graph itself is still what it was
    if name != "dropped":
        assert K >= 2
    if name == "wall":
        assert got["n_edges"] >= 1 and got["n_finite"].sum() > 0


# ---------------------------------------------------------------- several labels per node
def test_several_labels_per_node(gpu):
    xyz = big_boundary_voxel()
    eng = _vgs(gpu, xyz, **SPLIT)
    inp = _inputs(eng)
    n = xyz.shape[0]
    got = _check(eng, inp, np.arange(n) % 3, 3)
    pv = inp[0]
    full = [v for v in np.unique(pv[pv >= 0]) if np.unique((np.arange(n) % 3)[pv == v]).size == 3]
    assert got["seg_ab"].tolist() == [[0, 1], [0, 2], [1, 2]] and (got["n_shared"] == len(full)).all() and len(full) >= 4
    # between two nodes that carry all three labels every edge has two contacts
    off, idx = inp[1], inp[2]
    u = np.repeat(np.arange(off.shape[0] - 1), np.diff(off))
    both = np.isin(u, full) & np.isin(idx, full) & (u != idx)
    node_pairs = np.unique(np.minimum(u[both], idx[both]) * 10**6 + np.maximum(u[both], idx[both])).size
    assert node_pairs >= 2 and (got["n_pairs"] >= 2 * node_pairs).all()
    got70 = _check(eng, inp, np.arange(n) % 70, 70)   # more labels in one node than a wavefront has lanes
    assert got70["n_edges"] == 70 * 69 // 2 and got70["n_shared"].max() >= 3
    got7 = _check(eng, inp, np.arange(n) % 3, 7)   # empty labels behind
    assert all(got7[k].tobytes() == got[k].tobytes() for k in R.FIELDS)


# ---------------------------------------------------------------- unused endpoints, counted once
@pytest.mark.parametrize("params,pruned", [(GROUP5, False), (PRUNED5, True)], ids=["rows_hold_unused", "rows_pruned"])
def test_unused_endpoints_are_counted_once(gpu, params, pruned):
    xyz = dropped_beside_kept()
    eng = _vgs(gpu, xyz, **params)
    inp = _inputs(eng)
    assert _stored_rows_hold_unused(eng, inp) == (not pruned)
    kept = np.any([_voxel_of(xyz, (2 + i, 2, 2)) for i in range(4)], axis=0)
    b3, b4 = _voxel_of(xyz, (2, 2, 3)), _voxel_of(xyz, (2, 2, 4))
    top = np.any([_voxel_of(xyz, (2 + i, 2, 5)) for i in range(2)], axis=0)
    pv, used = inp[0], inp[3]
    assert used[np.unique(pv[kept | top])].all() and not used[np.unique(pv[b3 | b4])].any()
    labels = np.full(xyz.shape[0], -1, np.int32)
    labels[kept], labels[b3 | b4], labels[top] = 0, 1, 2
    got = _check(eng, inp, labels, 3)
    # lattice distances below graph_size = 0.25: five pairs between the kept row and the bridge, four between the bridge and the pair
    # above, none between the kept row and that pair (0.3); every one of them has an unused endpoint and so no weight
    assert got["seg_ab"].tolist() == [[0, 1], [1, 2]] and got["n_pairs"].tolist() == [5, 4] and got["n_finite"].tolist() == [0, 0]
    assert got["nodes_ab"].tolist() == [[3, 2], [2, 2]] and np.isnan(got["w_min"]).all() and (got["w_sum"] == 0).all()
    # the bridge split: one contact between two unused voxels; and a used / used edge beside it
    labels[b4] = 3
    labels[_voxel_of(xyz, (5, 2, 2))] = 4
    got = _check(eng, inp, labels, 5)
    e = {tuple(ab): i for i, ab in enumerate(got["seg_ab"].tolist())}
    assert got["n_pairs"][e[(1, 3)]] == 1 and got["n_finite"][e[(1, 3)]] == 0 and got["nodes_ab"][e[(1, 3)]].tolist() == [1, 1]
    assert got["n_pairs"][e[(0, 4)]] == 2 and got["n_finite"][e[(0, 4)]] == 2 and got["nodes_ab"][e[(0, 4)]].tolist() == [2, 1]
    assert got["n_pairs"][e[(0, 1)]] == 3 and got["n_pairs"][e[(0, 3)]] == 2 and (2, 4) not in e
    # several labels in unused and used voxels alike
    _check(eng, inp, np.where(np.isfinite(xyz).all(axis=1), np.arange(xyz.shape[0]) % 3, -1), 3)


# ---------------------------------------------------------------- reach
@pytest.mark.parametrize("shift,parts", [((3, 0, 0), 2), ((2, 0, 0), 1), ((2, 4, 0), 2), ((2, 3, 1), 1)],
                         ids=["two_steps", "one_step", "diagonal_above", "diagonal_below"])
def test_reach_between_two_slabs(gpu, shift, parts):
    """The slab pairs of test_gpu_label_components.py: the edge {0, 1} exists exactly where one labelling of both slabs is one part."""
    rng = np.random.default_rng(21)
    a = [(2, 2 + j, 2 + k) for j in range(3) for k in range(3)]
    b = [(2 + shift[0], 2 + j + shift[1], 2 + k + shift[2]) for j in range(3) for k in range(3)]
    if shift == (2, 3, 1):
        b = [(4, 5, 5)]
    xyz = np.concatenate([np.array([[0.1, 0.1, 0.1]])] + [_voxel_points(rng, v, 8) for v in a + b]).astype(np.float32)
    eng = _vgs(gpu, xyz, **GROUP5)
    labels = np.concatenate([[-1], np.zeros(8 * len(a)), np.ones(8 * len(b))]).astype(np.int32)
    got = _check(eng, _inputs(eng), labels, 2)
    assert eng.label_components(np.where(labels >= 0, 0, -1).astype(np.int32), 1)["n_parts"] == parts
    assert got["n_edges"] == (1 if parts == 1 else 0)
    if parts == 1:
        assert got["n_pairs"][0] >= 1 and got["n_shared"][0] == 0


# ---------------------------------------------------------------- row lengths
def test_rows_above_64_and_above_1024_entries(gpu):
    """The dense cube of test_gpu_label_components.py, with fewer used voxels (points_min = 7) so that the weights of every used pair stay
    cheap to restate: the stored rows exceed 64 entries, the rows built for unused voxels 1 024."""
    xyz = np.random.default_rng(12).uniform(0.0, 1.3, size=(12_000, 3)).astype(np.float32)
    eng = _vgs(gpu, xyz, voxel_size=0.1, graph_size=0.7, points_min=7, voxels_min=0)
    inp = _inputs(eng)
    rows, used = np.diff(inp[1]), inp[3]
    stored = max(eng.local_weights(int(v))[0].size for v in np.nonzero(used)[0][::20])
    assert used.sum() > 64 and (~used).any() and rows[~used].max() > 1024 and rows[used].max() > 1024 and stored > 64
    octant = (xyz[:, 0] > 0.65).astype(np.int32) + 2 * (xyz[:, 1] > 0.65) + 4 * (xyz[:, 2] > 0.65)
    octant[::7] = -1
    got = _check(eng, inp, octant, 8)
    assert got["n_edges"] == 28 and (got["n_shared"] > 0).any() and (got["n_finite"] > 0).all()


# ---------------------------------------------------------------- fold limits
def _strip(columns, rows, extra=0, per=8):
    """a one-voxel-thick slab of columns x rows voxels (plus `extra` voxels continuing column 0) with `per` points each; labels by column parity"""
    rng = np.random.default_rng(31)
    vox = [(2 + i, 2 + j, 2) for i in range(columns) for j in range(rows)] + [(2, 2 + rows + j, 2) for j in range(extra)]
    xyz = np.concatenate([np.array([[0.1, 0.1, 0.1]])] + [_voxel_points(rng, v, per) for v in vox]).astype(np.float32)
    labels = np.concatenate([[-1], np.repeat([v[0] % 2 for v in vox], per)]).astype(np.int32)
    return xyz, labels, len(vox)


def test_one_edge_of_20000_records(gpu):
    xyz, labels, n_vox = _strip(200, 100)
    eng = _vgs(gpu, xyz, **GROUP5)
    got = _check(eng, _inputs(eng), labels, 2)
    # every voxel is one vertex with one record: more than LG_CHUNK records in a chunk's edge and more than 64 chunks (the lane stride of k_lg_final)
    assert n_vox == 20_000 > 64 * LG_CHUNK and got["n_edges"] == 1 and got["nodes_ab"].tolist() == [[10_000, 10_000]]
    assert got["n_pairs"][0] > 3 * n_vox and got["n_finite"][0] > 0


@pytest.mark.parametrize("extra", [0, 1], ids=["256_records", "257_records"])
def test_an_edge_of_one_chunk_and_of_one_record_more(gpu, extra):
    xyz, labels, n_vox = _strip(2, 128, extra)
    eng = _vgs(gpu, xyz, **GROUP5)
    got = _check(eng, _inputs(eng), labels, 2)
    assert n_vox == LG_CHUNK + extra and got["n_edges"] == 1 and int(got["nodes_ab"].sum()) == n_vox


# ---------------------------------------------------------------- key range
def test_key_of_40_bits(gpu):
    rng = np.random.default_rng(5)
    K = 1 << 20
    xyz = np.concatenate([np.array([[0.1, 0.1, 0.1]])] + [_voxel_points(rng, (2 + i, 2, 2), 8) for i in range(3)]).astype(np.float32)
    labels = np.concatenate([[-1], np.repeat([K - 1, 0, 5], 8)]).astype(np.int32)
    eng = _vgs(gpu, xyz, **GROUP5)
    got = _check(eng, _inputs(eng), labels, K)
    # the sort runs over the 40 bits of the key space K * K; the three voxels lie within graph_size of each other
    assert got["seg_ab"].tolist() == [[0, 5], [0, K - 1], [5, K - 1]] and got["n_pairs"].tolist() == [1, 1, 1]


# ---------------------------------------------------------------- edge inputs
def test_edge_inputs(gpu):
    xyz = dropped_beside_kept()
    eng = _vgs(gpu, xyz, **GROUP5)
    inp = _inputs(eng)
    n = xyz.shape[0]
    finite = np.isfinite(xyz).all(axis=1)
    cases = [(np.full(n, -1, np.int32), 0, 0), (np.zeros(n, np.int32), 1, 4), (np.full(n, -1, np.int32), 3, 0), (np.full(n, -7, np.int32), 1, 0),
             (np.where(finite, -1, 2).astype(np.int32), 3, 4),      # labels only on the points outside the octree
             (np.full(n, 2, np.int32), 5, 4)]                         # one label only
    for labels, K, skipped in cases:
        got = _check(eng, inp, labels, K)
        assert got["n_edges"] == 0 and got["n_skipped"] == skipped and all(got[k].shape[0] == 0 for k in R.FIELDS)
        assert eng.label_graph_device() == (0, {k: None for k in R.FIELDS})
    assert eng.label_graph(np.full(n, -1, np.int32))["n_edges"] == 0   # K None of an all-negative labelling: 0
    two = np.where(finite, np.arange(n) % 2, 1).astype(np.int32)       # labelled NaN points beside a real graph
    assert _check(eng, inp, two, 2)["n_skipped"] == 4


@pytest.mark.parametrize("kind", ["no_finite_point", "empty_cloud"])
def test_clouds_without_a_node(gpu, kind):
    xyz = np.full((5, 3), np.nan, np.float32) if kind == "no_finite_point" else np.zeros((0, 3), np.float32)
    eng = _vgs(gpu, xyz, **GROUP5)
    n = xyz.shape[0]
    got = eng.label_graph((np.arange(n) % 2).astype(np.int32), 2)
    assert got["n_edges"] == 0 and got["n_skipped"] == n and all(got[k].shape[0] == 0 for k in R.FIELDS)


# ---------------------------------------------------------------- SVGS
def test_svgs_mirror_pair_and_grid_supervoxels(gpu):
    xyz, sv, mx = mirror_pair()
    eng = _svgs(gpu, xyz, sv, mx)
    inp = _inputs(eng)
    n = xyz.shape[0]
    _check(eng, inp, eng.point_labels(), eng.counts()["kept"])
    assert _check(eng, inp, np.arange(n) % 2, 2)["n_shared"][0] >= 3   # alternating inside the supervoxels
    assert _check(eng, inp, np.maximum(sv - 1, -1), mx)["n_edges"] >= 1   # every supervoxel a label of its own
    xyz = blob(n=6000)
    sv, mx = grid_supervoxels(xyz)
    eng = _svgs(gpu, xyz, sv, mx)
    inp = _inputs(eng)
    own = _check(eng, inp, eng.point_labels(), eng.counts()["kept"])
    seg = eng.segment_graph()
    assert all(own[k].tobytes() == seg[k].tobytes() for k in ("seg_ab", "n_pairs", "n_finite", "nodes_ab", "w_min", "w_max"))
    got = _check(eng, inp, (xyz[:, 0] > 0).astype(np.int32) + (xyz[:, 1] > 0.4), 3)
    assert got["n_edges"] == 3 and (got["n_shared"] > 0).any()


# ---------------------------------------------------------------- composition
_cube = {}


def _cube_scene(gpu):
    if not _cube:
        xyz = np.random.default_rng(8).uniform(0.0, 1.2, size=(6_000, 3)).astype(np.float32)
        eng = _vgs(gpu, xyz, **GROUP5)
        _cube.update(xyz=xyz, eng=eng, inp=_inputs(eng))
    return _cube["xyz"], _cube["eng"], _cube["inp"]


def test_graph_of_the_parts_of_a_labelling(gpu):
    xyz, eng, inp = _cube_scene(gpu)
    used = inp[3]
    assert used.any() and not used.all()
    K = 3
    # stripes of 0.25 along x, labels 0 1 2 0 1: labels 0 and 1 have two parts each, 0.5 apart; the borders run through the voxels
    labels = (np.floor(xyz[:, 0] / 0.25).astype(np.int32) % K).astype(np.int32)
    labels[::11] = -1
    whole = _check(eng, inp, labels, K)
    parts = eng.label_components(labels, K)
    P = parts["n_parts"]
    assert P > K
    got = _check(eng, inp, parts["part_of_point"], P)   # an edge exactly where the restatement finds a contact or a shared node
    la, lb = parts["part_label"][got["seg_ab"][:, 0]], parts["part_label"][got["seg_ab"][:, 1]]
    assert (la != lb).all()   # two parts of one label never touch
    # the additive fields summed over the parts of each label pair give the graph of the labelling itself (a vertex can be in contacts
    # with several parts of the other label, so nodes_ab is not additive)
    key = np.minimum(la, lb).astype(np.int64) * K + np.maximum(la, lb)
    keys, inv = np.unique(key, return_inverse=True)
    assert np.array_equal(np.stack([keys // K, keys % K], axis=1), whole["seg_ab"])
    for k in ("n_shared", "n_pairs", "n_finite"):
        assert np.array_equal(np.bincount(inv, weights=got[k], minlength=keys.size).astype(np.int64), whole[k]), k
    s = np.bincount(inv, weights=got["w_sum"], minlength=keys.size)
    assert (np.abs(s - whole["w_sum"]) <= 1e-10 * np.abs(whole["w_sum"])).all()
    mn = np.full(keys.size, np.inf, np.float32)
    np.fmin.at(mn, inv, got["w_min"])
    assert np.array_equal(mn[whole["n_finite"] > 0], whole["w_min"][whole["n_finite"] > 0])


def test_graph_of_the_refined_labels(gpu):
    xyz = floor_and_wall()[0]
    eng = _vgs(gpu, xyz, **WALL)
    eng.refine_labels()
    refined, K = eng.refined_labels(), eng.counts()["kept"]
    got = _check(eng, _inputs(eng), refined, K)
    assert K >= 2 and got["n_edges"] >= 1 and got["n_shared"].max() > 0   # boundary voxels hold two labels
    assert np.array_equal(eng.refined_labels(), refined)   # the refinement's own buffer is untouched


# ---------------------------------------------------------------- determinism and input forms
def test_determinism_and_input_forms(gpu):
    torch = pytest.importorskip("torch")
    xyz, eng, inp = _cube_scene(gpu)
    n = xyz.shape[0]
    labels = np.random.default_rng(3).integers(-1, 9, size=n).astype(np.int32)
    seg, own, comp = eng.segment_graph(), eng.point_labels(), eng.label_components(labels, 9)
    a = eng.label_graph(labels, 9)
    assert a["n_edges"] == 36 and (a["n_shared"] > 0).any()

    def same(x):
        return x["n_edges"] == a["n_edges"] and x["n_skipped"] == a["n_skipped"] and all(x[k].tobytes() == a[k].tobytes() for k in R.FIELDS)

    assert same(eng.label_graph(labels, 9))
    assert same(_vgs(gpu, xyz, **GROUP5).label_graph(labels, 9))
    dev = torch.from_numpy(labels).to("cuda:0")
    assert same(eng.label_graph(dev, 9)) and same(eng.label_graph(dev))   # K None on the device: max + 1
    # the device-pointer variant reads back the same table
    E, ptrs = eng.label_graph_device()
    assert E == a["n_edges"] and all(ptrs.values())
    hip = C.cdll.LoadLibrary("libamdhip64.so")
    for name, dt, w in gpu.Engine.LABEL_GRAPH_FIELDS:
        back = np.zeros((E, w) if w > 1 else E, dtype=dt)
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(ptrs[name]), C.c_size_t(back.nbytes), 2) == 0
        assert back.tobytes() == a[name].tobytes(), name
    eng._ck(eng._L.vgs_get_point_label_graph(eng._h, *([None] * 8)))   # any pointer may be NULL
    # the other results are untouched by the calls
    seg2 = eng.segment_graph()
    assert all(seg2[k].tobytes() == seg[k].tobytes() for k in seg) and np.array_equal(eng.point_labels(), own)
    out = {name: np.zeros(comp[name].shape, comp[name].dtype) for name, _, _ in gpu.Engine.COMPONENT_FIELDS}
    eng._ck(eng._L.vgs_get_point_label_components(eng._h, *(out[name].ctypes.data_as(C.c_void_p) for name, _, _ in gpu.Engine.COMPONENT_FIELDS)))
    assert all(out[name].tobytes() == comp[name].tobytes() for name in out)
    # ... and a components call in between leaves the graph where it is
    eng.label_components(labels, 9)
    assert eng.label_graph_device() == (E, ptrs)


# ---------------------------------------------------------------- the status contract
def test_status_contract(gpu):
    lib = gpu._lib
    xyz = dropped_beside_kept()
    n = xyz.shape[0]
    labels = (np.arange(n) % 2).astype(np.int32)
    eng = gpu.Engine(gpu.default_params(2, **GROUP5))
    eng.set_points(xyz)

    def fails(call, status):
        with pytest.raises(gpu.VgsError) as e:
            call()
        assert e.value.status == status, e.value
        return str(e.value)

    fails(lambda: eng.label_graph(labels, 2), lib.VGS_E_STATE)   # before a run
    eng.run()
    fails(eng.label_graph_device, lib.VGS_E_STATE)   # the getters before a compute call
    fails(lambda: eng._ck(eng._L.vgs_get_point_label_graph(eng._h, *([None] * 8))), lib.VGS_E_STATE)
    fails(lambda: eng.label_graph(labels[:-1], 2), lib.VGS_E_ARG)   # n != N
    fails(lambda: eng._ck(eng._L.vgs_point_label_graph(eng._h, None, n, 2, None, None)), lib.VGS_E_ARG)   # NULL labels
    fails(lambda: eng._ck(eng._L.vgs_point_label_graph(eng._h, labels.ctypes.data_as(C.c_void_p), n, -1, None, None)), lib.VGS_E_ARG)
    fails(lambda: eng._ck(eng._L.vgs_point_label_graph(eng._h, labels.ctypes.data_as(C.c_void_p), n, 1 << 31, None, None)), lib.VGS_E_ARG)
    bad = labels.copy()
    bad[7], bad[11] = 3, 9
    msg = fails(lambda: eng.label_graph(bad, 3), lib.VGS_E_ARG)   # a label >= K: the first offending index
    assert "labels[7] = 3" in msg
    fails(eng.label_graph_device, lib.VGS_E_STATE)   # ... and it left no result behind
    assert eng.label_graph(labels, 2)["n_edges"] == 1
    eng.label_graph_device()
    eng.run()   # a new run of the stages
    fails(eng.label_graph_device, lib.VGS_E_STATE)
    # a tile context is refused, the limitation named
    t = gpu.Engine(gpu.default_params(2, **GROUP5))
    t.set_points(xyz)
    lo, hi = np.array([-1e9, -1e9], dtype=np.float64), np.array([1e9, 1e9], dtype=np.float64)
    t._ck(t._L.vgs_set_owned_region(t._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    t.run()
    msg = fails(lambda: t.label_graph(labels, 2), lib.VGS_E_STATE)
    assert "tile context" in msg and "across the ranks" in msg and "not computed" in msg
    assert "across the ranks" in fails(t.label_graph_device, lib.VGS_E_STATE)
