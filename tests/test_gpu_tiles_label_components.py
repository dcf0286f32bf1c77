"""Connected parts of any per-point labelling across the ranks of the native tiled driver (vgs_tiles_point_label_components,
include/vgs_tiles.h), ranks as threads of this process over LocalGroup on one GPU.  Every rank hands in the labels of its own points; band
records, local parts and link triples cross, no point and no label.

The oracle is ONE plain Engine on np.concatenate(parts) -- rank order, the order the shared grid is chained in -- and its
label_components(), which tests/test_gpu_label_components.py holds to tests/label_components_ref.py.  Everything is integer: part_of_point
(concatenated over the ranks), part_label, part_points, part_nodes, label_first, label_largest and the two counts are compared by bytes.
part_first_code is compared with attribute_scenes._morton(voxel_table()["key"])[part_first_node]: the shared grid's code is that
interleave of the plain engine's key (bit triple x << 2 | y << 1 | z, what tile_region.hpp's rf_center takes apart).

Designed scenes are built on the voxel lattice through the origin (voxel_size 0.1; the first point of rank 0, on a lattice corner, fixes
the octree's first box) and split by region; every case asserts a precondition on the plain engine so that it cannot pass vacuously."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from attribute_scenes import _morton
from label_refine_scenes import GROUP5, _voxel_points
from segment_scenes import GROUP
from test_gpu_tiles_point_label_tables import _mixed_labels, _offsets
from test_gpu_tiles_refine import _Meet
from test_gpu_tiles_segdesc import _parts, _pitch, _ranks, _same
from test_gpu_tiles_segfields import LAYOUTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")
N_PER = 60_000
TABLES = ("part_label", "part_points", "part_nodes", "label_first", "label_largest")
ALL = ("part_of_point",) + TABLES + ("part_first_code",)
LT_SHORT = 64           # rows up to so many entries share a wavefront (csrc/labelcc_tiles.hip)
CC_HEADER = 4           # words of 8 bytes in front of each of the two payloads
# rows pruned to used neighbours (the default cut threshold), voxels of at most five points unused
PRUNED5 = dict(voxel_size=0.1, graph_size=0.25, points_min=5, voxels_min=0)
ANCHOR = np.array([[0.1, 0.1, 0.1]])


# ---------------------------------------------------------------- helpers
def _engine(gpu, xyz, kw):
    eng = gpu.Engine(gpu.default_params(2, **kw))
    eng.set_points(xyz)
    eng.run()
    return eng


def _cells(rng, cells, n=12):
    return np.concatenate([_voxel_points(rng, c, n) for c in cells])


def _split(xyz, lab, tiles, center):
    """the points and labels of every rank, loaded by region: tile (i, j) of the layout, outer tiles open ended (vgs_tiles_create)"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    x, y = xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)
    i = (x >= center[0]).astype(np.int64) if tiles[0] == 2 else np.zeros(x.size, np.int64)
    j = (y >= center[1]).astype(np.int64) if tiles[1] == 2 else np.zeros(x.size, np.int64)
    rank = j * tiles[0] + i
    world = tiles[0] * tiles[1]
    return [xyz[rank == r] for r in range(world)], [np.ascontiguousarray(lab[rank == r], dtype=np.int32) for r in range(world)]


def _body(labs, K, own=True):
    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        c = t.label_components(labs[r], K)
        res = dict(c=c, pay=t.label_component_payload(), times=t.label_component_times())
        if own:
            res["own"] = t.own_point_label_parts(labs[r], K)
        return res
    return body


def _against_engine(eng, labs, K, out):
    """the tiled result of every rank against the plain engine's on the gathered points"""
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    want = eng.label_components(np.concatenate(labs), K)
    got = out[0]["c"]
    for o in out[1:]:
        for name in TABLES + ("part_first_code",):
            assert o["c"][name].tobytes() == got[name].tobytes(), name      # every rank: the same bytes
        assert o["c"]["n_parts"] == got["n_parts"] and o["c"]["n_skipped"] == got["n_skipped"]
    pop = np.concatenate([o["c"]["part_of_point"] for o in out])
    assert pop.dtype == want["part_of_point"].dtype and pop.tobytes() == want["part_of_point"].tobytes()
    for name in TABLES:
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), (name, got[name], want[name])
    assert got["n_parts"] == want["n_parts"] and got["n_skipped"] == want["n_skipped"]
    code = _morton(eng.voxel_table()["key"])
    assert got["part_first_code"].dtype == np.uint64 and np.array_equal(got["part_first_code"], code[want["part_first_node"]])
    return want


def _designed(gpu, xyz, lab, K, tiles, center, kw, own=True):
    parts, labs = _split(xyz, lab, tiles, center)
    assert all(p.shape[0] > 0 for p in parts) and np.array_equal(parts[0][0], ANCHOR[0].astype(np.float32))
    out = _ranks(gpu, tiles, 4.0, parts, _body(labs, K, own), center=center, params=gpu.default_params(2, **kw), timeout=120.0)
    eng = _engine(gpu, np.concatenate(parts), kw)
    want = _against_engine(eng, labs, K, out)
    return out, want, eng, parts, labs


def _with_anchor(xyz, lab):
    return np.concatenate([ANCHOR, xyz]).astype(np.float32), np.concatenate([[-1], lab]).astype(np.int32)


def _voxel_id(eng, ijk):
    key = eng.voxel_table()["key"].astype(np.int64)
    cen = eng.voxel_centers().astype(np.float64)
    want = (np.asarray(ijk, dtype=np.float64) + 0.5) * 0.1
    v = np.flatnonzero(np.abs(cen - want).max(axis=1) < 0.01)
    assert v.size == 1, (ijk, v, key.shape)
    return int(v[0])


# ---------------------------------------------------------------- 1. designed scenes, 2x1 (the border is the plane x = center[0])
def test_row_across_the_border_is_one_part(gpu):
    rng = np.random.default_rng(1)
    xyz, lab = _with_anchor(_cells(rng, [(i, 2, 2) for i in range(10, 30)]), np.zeros(20 * 12))
    out, want, _, _, _ = _designed(gpu, xyz, lab, 1, (2, 1), (2.0, 0.0), GROUP)
    assert want["n_parts"] == 1 and want["part_nodes"].tolist() == [20]
    assert all((o["c"]["part_of_point"] == 0).sum() == 120 for o in out)                 # points of the one part on both ranks
    assert all(o["pay"]["band_records"] > 0 and o["pay"]["links"] > 0 for o in out)


def test_gap_wider_than_graph_size_at_the_border_gives_two_parts(gpu):
    rng = np.random.default_rng(2)
    cells = [(i, 2, 2) for i in range(10, 16)] + [(i, 2, 2) for i in range(24, 30)]      # 15 and 24: 0.9 apart, graph_size 0.5
    xyz, lab = _with_anchor(_cells(rng, cells), np.zeros(12 * 12))
    out, want, _, _, _ = _designed(gpu, xyz, lab, 1, (2, 1), (2.0, 0.0), GROUP)
    assert want["n_parts"] == 2 and want["part_points"].tolist() == [72, 72]
    assert out[1]["c"]["part_of_point"].tolist() == [0] * 72 and out[0]["c"]["part_of_point"].tolist() == [-1] + [1] * 72


@pytest.mark.parametrize("same", [True, False], ids=["same_label", "two_labels"])
def test_voxel_cut_by_the_border(gpu, same):
    """the border x = 2.05 cuts the voxel 20 of a row of five: under one label one part whose nodes count the voxel once; with the points
    of the two ranks under different labels two parts that share the voxel"""
    rng = np.random.default_rng(3)
    pts = _cells(rng, [(i, 2, 2) for i in range(18, 23)], n=40)
    lab = np.zeros(pts.shape[0]) if same else (pts[:, 0].astype(np.float32).astype(np.float64) >= 2.05).astype(np.int64)
    xyz, lab = _with_anchor(pts, lab)
    out, want, eng, parts, _ = _designed(gpu, xyz, lab, 2, (2, 1), (2.05, 0.0), GROUP)
    cut = [int(((np.floor(p[:, 0] / np.float32(0.1)) == 20) & (p[:, 1] > 0.15)).sum()) for p in parts]
    assert min(cut) > 0 and sum(cut) == 40, cut                                            # the voxel holds points of both ranks
    if same:
        assert want["n_parts"] == 1 and want["part_nodes"].tolist() == [5] and want["part_points"].tolist() == [200]
        assert sum(int(o["own"]["part_nodes"].sum()) for o in out) == 6                    # ... and each rank counts it
    else:
        assert want["n_parts"] == 2 and want["part_label"].tolist() == [0, 1] and want["part_nodes"].tolist() == [3, 3]
    shared = [set(o["own"]["band_code"].tolist()) for o in out]
    assert len(shared[0] & shared[1]) == 1


def test_used_voxel_beside_an_unused_voxel_of_the_other_rank(gpu):
    """rows pruned to used neighbours: the stored row of the used voxel 19 (rank 0) lacks the unused voxel 20 (three points, rank 1); the
    edge comes from the full row built for 20 on rank 1"""
    rng = np.random.default_rng(4)
    pts = np.concatenate([_cells(rng, [(18, 2, 2), (19, 2, 2)], n=30), _voxel_points(rng, (20, 2, 2), 3)])
    xyz, lab = _with_anchor(pts, np.zeros(pts.shape[0]))
    out, want, eng, _, _ = _designed(gpu, xyz, lab, 1, (2, 1), (2.0, 0.0), PRUNED5)
    v19, v20 = _voxel_id(eng, (19, 2, 2)), _voxel_id(eng, (20, 2, 2))
    used = eng.attributes()["used"]
    assert used[v19] and not used[v20]
    off, idx = eng.lists("adjacency")
    assert v20 in idx[off[v19]:off[v19 + 1]] and v19 in idx[off[v20]:off[v20 + 1]]
    assert v20 not in eng.local_weights(v19)[0].tolist() and v19 in eng.local_weights(v19)[0].tolist()   # the stored row is pruned
    assert want["n_parts"] == 1 and want["part_points"].tolist() == [63] and want["part_nodes"].tolist() == [3]
    assert out[1]["c"]["part_of_point"].tolist() == [0, 0, 0]


def _zigzag(z):
    """nine rows across the border (x = 2.0, between the voxels 19 and 20), four voxels apart in y, joined at alternating ends"""
    cells = []
    for k in range(9):
        y = 2 + 4 * k
        cells += [(i, y, z) for i in range(17, 23)]
        if k < 8:
            cells += [(22 if k % 2 == 0 else 17, y + d, z) for d in (1, 2, 3)]
    return cells


def test_zigzag_that_leaves_a_rank_and_comes_back(gpu):
    rng = np.random.default_rng(5)
    a, b = _zigzag(2), _zigzag(12)
    xyz, lab = _with_anchor(_cells(rng, a + b, n=8), np.zeros(8 * (len(a) + len(b))))
    out, want, _, _, _ = _designed(gpu, xyz, lab, 1, (2, 1), (2.0, 0.0), GROUP5)
    assert want["n_parts"] == 2 and want["part_nodes"].tolist() == [len(a), len(b)]        # the second zigzag keeps its own id
    for o in out:
        assert o["own"]["part_label"].size >= 2 * 4                                          # at least four local parts per zigzag and rank
        assert set(o["c"]["part_of_point"].tolist()) - {-1} == {0, 1}
    assert out[0]["own"]["part_label"].size == out[1]["own"]["part_label"].size == 10


def test_numbering_is_by_code_not_by_rank(gpu):
    """two parts of one label with equal point counts; the one with the smaller node id (the larger code) lies on rank 1"""
    rng = np.random.default_rng(6)
    cells = [(i, 2, 2) for i in range(5, 9)] + [(i, 2, 2) for i in range(30, 34)]
    xyz, lab = _with_anchor(_cells(rng, cells), np.zeros(8 * 12))
    out, want, _, _, _ = _designed(gpu, xyz, lab, 1, (2, 1), (2.0, 0.0), GROUP)
    assert want["n_parts"] == 2 and want["part_points"].tolist() == [48, 48] and want["part_first_node"][0] < want["part_first_node"][1]
    assert out[1]["c"]["part_of_point"].tolist() == [0] * 48 and out[0]["c"]["part_of_point"].tolist() == [-1] + [1] * 48
    assert want["label_largest"].tolist() == [0]
    assert out[0]["c"]["part_first_code"][0] > out[0]["c"]["part_first_code"][1]


@pytest.mark.parametrize("kind", ["long_rows", "short_rows"])
def test_both_row_widths_of_the_link_kernel(gpu, kind):
    rng = np.random.default_rng(7)
    if kind == "long_rows":      # a block of 10 x 6 x 4 voxels across the border, graph_size 0.5
        cells, kw = [(i, j, k) for i in range(15, 25) for j in range(3, 9) for k in range(3, 7)], GROUP
    else:                        # two rows of voxels, graph_size 0.25
        cells, kw = [(i, j, 3) for i in range(12, 28) for j in (3, 4)], GROUP5
    xyz, lab = _with_anchor(_cells(rng, cells, n=8), np.zeros(8 * len(cells)))
    out, want, eng, _, _ = _designed(gpu, xyz, lab, 1, (2, 1), (2.0, 0.0), kw)
    off, _ = eng.lists("adjacency")
    rows = np.diff(off)[[_voxel_id(eng, c) for c in cells if 18 <= c[0] <= 21]]            # the voxels next to the border: in the band
    assert (rows.min() > LT_SHORT + 1) if kind == "long_rows" else (rows.max() <= LT_SHORT), (rows.min(), rows.max())
    assert want["n_parts"] == 1 and want["part_nodes"].tolist() == [len(cells)]
    assert all(o["pay"]["links"] > 0 for o in out)


# ---------------------------------------------------------------- 2. designed scenes, 2x2 (borders x = 2.05 and y = 2.05)
def test_corner_ring_and_chain_through_four_ranks(gpu):
    """label 0: a ring around the corner through all four ranks; label 1: the corner voxel (20, 20, 9), points of all four ranks, one
    node; label 2: a chain rank 0 - rank 1 - rank 3, ranks 0 and 3 sharing no band record"""
    rng = np.random.default_rng(8)
    ring = [(i, j, 2) for i in range(17, 24) for j in range(17, 24) if i in (17, 23) or j in (17, 23)]
    quad = np.array([[2.0 + 0.01 + 0.03 * a + 0.05 * sx, 2.0 + 0.01 + 0.03 * b + 0.05 * sy, 0.95] for sx in (0, 1) for sy in (0, 1) for a in (0, 1) for b in (0, 1)])
    chain = [(i, 10, 15) for i in range(15, 31)] + [(30, j, 15) for j in range(11, 31)]
    pts = np.concatenate([_cells(rng, ring, n=8), quad, _cells(rng, chain, n=8)])
    lab = np.concatenate([np.zeros(8 * len(ring)), np.ones(16), np.full(8 * len(chain), 2)])
    xyz, lab = _with_anchor(pts, lab)
    out, want, eng, parts, labs = _designed(gpu, xyz, lab, 3, (2, 2), (2.05, 2.05), GROUP5)
    assert want["n_parts"] == 3 and want["part_label"].tolist() == [0, 1, 2]
    assert want["part_nodes"].tolist() == [len(ring), 1, len(chain)] and want["part_points"].tolist() == [8 * len(ring), 16, 8 * len(chain)]
    assert all(int((l == 1).sum()) == 4 for l in labs)                                      # the corner voxel: four points of every rank
    assert all(int((l == 0).sum()) > 0 for l in labs)                                       # the ring passes through all four
    assert [int((l == 2).sum()) > 0 for l in labs] == [True, True, False, True]
    band = [set(zip(o["own"]["band_code"].tolist(), o["own"]["band_label"].tolist())) for o in out]
    corner = band[0] & band[1] & band[2] & band[3]
    assert len(corner) == 1 and next(iter(corner))[1] == 1                                  # one key published by all four ranks
    b0 = {c for c, l in band[0] if l == 2}
    b3 = {c for c, l in band[3] if l == 2}
    assert b0 and b3 and not (b0 & b3)


# ---------------------------------------------------------------- 3. labellings on the urban layouts
@pytest.mark.parametrize("layout", ["2x1", "2x2", "2x2_far"])
def test_layouts_match_one_engine_over_the_gathered_points(gpu, layout):
    import torch
    tiles, shift = LAYOUTS[layout]
    parts = _parts(gpu, tiles, N_PER, shift)
    bad = np.array([[np.nan, 1.0, 1.0]], np.float32)
    parts = [np.concatenate([p, bad]) for p in parts]   # one point per rank outside the octree, labelled below
    off = _offsets(parts)
    world = len(parts)

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        pl, kept = t.point_labels()
        t.refine_labels()
        fine = t.refined_labels().copy()
        n = xyz.shape[0]
        one = np.zeros(n, np.int32)
        only = np.where(np.arange(n) % 3 == 0, 0, -1).astype(np.int32) if r == world - 1 else np.full(n, -1, np.int32)
        cases = dict(own=(pl, kept), refined=(fine, kept), mixed=(_mixed_labels(pl, off[r], 1), 2 * kept + 3), one=(one, 1),
                     none=(np.full(n, -7, np.int32), 4), k0=(np.full(n, -1, np.int32), 0), one_rank_only=(only, 2))
        res = {name: dict(lab=lab, K=K, c=t.label_components(lab, K)) for name, (lab, K) in cases.items()}
        if layout == "2x1":
            lab, K = cases["mixed"]
            dev = t.label_components(torch.as_tensor(lab, device=f"cuda:{t.params.device}"), K)
            res["device_equal"] = all(dev[k].tobytes() == res["mixed"]["c"][k].tobytes() for k in ALL) and dev["n_skipped"] == res["mixed"]["c"]["n_skipped"]
        return res
    center = tuple(shift[:2]) if shift else (0.0, 0.0)
    out = _ranks(gpu, tiles, _pitch(N_PER), parts, body, center=center)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    eng = _engine(gpu, np.concatenate(parts), dict(voxel_size=0.1))
    for name in ("own", "refined", "mixed", "one", "none", "k0", "one_rank_only"):
        K = out[0][name]["K"]
        assert all(o[name]["K"] == K for o in out)
        want = _against_engine(eng, [o[name]["lab"] for o in out], K, [dict(c=o[name]["c"]) for o in out])
        print(layout, name, K, want["n_parts"], want["n_skipped"])
        if name in ("none", "k0"):
            assert want["n_parts"] == 0 and all((o[name]["c"]["part_of_point"] == -1).all() for o in out)
        else:
            assert want["n_parts"] > 0
    assert out[0]["mixed"]["c"]["n_skipped"] == world and all(o["mixed"]["c"]["part_of_point"][-1] == -1 for o in out)   # the NaN points
    assert out[0]["own"]["c"]["n_parts"] >= out[0]["own"]["K"] > 0
    if layout == "2x1":
        assert all(o["device_equal"] for o in out)


def test_one_id_per_point(gpu):
    parts = _parts(gpu, (2, 1), 1000)
    off = _offsets(parts)
    n = int(off[-1])
    labs = [np.arange(off[r], off[r + 1], dtype=np.int32) for r in range(2)]
    out = _ranks(gpu, (2, 1), _pitch(1000), parts, _body(labs, n, own=False), timeout=120.0)
    want = _against_engine(_engine(gpu, np.concatenate(parts), dict(voxel_size=0.1)), labs, n, out)
    assert want["n_parts"] + want["n_skipped"] == n == 2000


# ---------------------------------------------------------------- 4. one rank
def test_one_rank_equals_a_plain_engine_with_two_exchanges_per_call(gpu):
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
        pl, kept = t.point_labels()
        lab = _mixed_labels(pl, 0, 0)
        before = dict(calls)
        got = t.label_components(lab, 2 * kept + 3)
        # two all_gather_varlen: the sizes and the padded payload each
        assert (calls["ag"] - before["ag"], calls["bc"] - before["bc"]) == (4, 0), (before, calls)
        assert t.label_component_payload() == dict(band_records=0, parts=got["n_parts"], links=0, bytes_sent=8 * (2 * CC_HEADER + 3 * got["n_parts"]))
        eng = _engine(gpu, xyz, dict(voxel_size=0.1))
        _against_engine(eng, [lab], 2 * kept + 3, [dict(c=got)])
    finally:
        t.close()


# ---------------------------------------------------------------- 5. protocol
def test_protocol_payload_determinism_and_side_effects(gpu):
    from vgs_svgs_segmentation_amd import tiles_native as tn
    tiles = (2, 1)
    parts = _parts(gpu, tiles, N_PER)    # (at 20 000 points per rank the scene keeps one segment, none of it near the border)
    off = _offsets(parts)
    meet = _Meet(2)
    sync = threading.Barrier(2)
    shared = [None, None]
    out = [None, None]

    def tables(t, ref, kept):
        c = t.compare_labels(ref)
        return dict(d=t.segment_descriptors(), b=t.segment_boxes("upright"), g=t.segment_graph(), c=c)

    def cached(t, c, kept):
        return dict(d=t.segment_descriptors(), b=t.segment_boxes("upright"), g=t.segment_graph(),
                    c=t.label_comparison(c["cell_n"].size, c["ref_id"].size, kept))

    def same_tables(a, b):
        return _same(a["d"], b["d"]) and _same(a["b"], b["b"]) and _same(a["g"], b["g"]) and all(
            np.array_equal(a["c"][k], b["c"][k]) for k in b["c"] if k != "summary")

    def rank_main(r):
        try:
            ag, bc = meet.callbacks(r)
            t = tn.NativeTiles.with_callbacks(gpu.default_params(2, voxel_size=0.1), r, 2, tiles, _pitch(N_PER), ag, bc)
            try:
                t.set_points(parts[r])
                t.run()
                pl, kept = t.point_labels()
                lab, K = _mixed_labels(pl, off[r], 0), 2 * kept + 3
                ref = np.ascontiguousarray(((off[r] + np.arange(parts[r].shape[0])) // 97 % 23 - 1).astype(np.int32))
                before = dict(meet.calls[r])
                first = t.label_components(lab, K)                      # before any cached table exists
                n_ag = (meet.calls[r]["ag"] - before["ag"], meet.calls[r]["bc"] - before["bc"])
                pay = t.label_component_payload()
                t.refine_labels()
                fine = t.refined_labels().copy()
                A = tables(t, ref, kept)
                second = t.label_components(lab, K)                     # behind them
                B = cached(t, A["c"], kept)
                fine_after = t.refined_labels().copy()
                before = dict(meet.calls[r])
                getter = t.label_components_result(second["n_parts"], K)   # not collective
                n_get = meet.calls[r]["ag"] - before["ag"]
                t.run()
                third = t.label_components(lab, K)
                own = t.own_point_label_parts(lab, K)
                shared[r] = own
                sync.wait(60)
                o = shared[1 - r]
                own.update(t.link_point_label_parts(o["band_code"], o["band_label"], np.full(o["band_label"].size, 1 - r, np.int32), o["band_part"]))
                out[r] = dict(first=first, second=second, third=third, getter=getter, n_ag=n_ag, n_get=n_get, pay=pay, own=own, K=K,
                              side=same_tables(A, B) and np.array_equal(fine, fine_after), times=t.label_component_times())
            finally:
                t.close()
        except Exception as ex:  # noqa: BLE001
            out[r] = ex
            sync.abort()
            meet.barrier.abort()
    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join(300.0)
    assert not any(x.is_alive() for x in th)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    for o in out:
        assert o["n_ag"] == (4, 0) and o["n_get"] == 0          # two all_gather_varlen, each the sizes and the padded payload
        for name in ALL:
            assert o["first"][name].tobytes() == o["second"][name].tobytes() == o["third"][name].tobytes() == o["getter"][name].tobytes(), name
        assert o["side"]
        own, pay = o["own"], o["pay"]
        assert pay["band_records"] == own["band_code"].size > 0 and pay["parts"] == own["part_label"].size > 0 and pay["links"] == own["link_own"].size > 0
        assert pay["bytes_sent"] == 8 * (2 * CC_HEADER + 2 * pay["band_records"] + 3 * pay["parts"] + 2 * pay["links"])
        assert set(o["times"]) == {"own", "exchange1", "link", "exchange2", "fold", "apply", "total"} and o["times"]["total"] > 0
    for name in TABLES + ("part_first_code",):
        assert out[0]["first"][name].tobytes() == out[1]["first"][name].tobytes(), name
    # the own records, folded, give the table
    folded = tn.fold_label_parts([o["own"] for o in out], out[0]["K"])
    for name in TABLES + ("part_first_code",):
        assert folded[name].tobytes() == out[0]["first"][name].tobytes(), name
    assert folded["n_parts"] == out[0]["first"]["n_parts"]


# ---------------------------------------------------------------- 6. the status contract
def test_before_a_run_and_before_a_call(gpu):
    from vgs_svgs_segmentation_amd import tiles_native as tn
    grp = tn.LocalGroup(2)
    t = tn.NativeTiles(gpu.default_params(2, voxel_size=0.1), tn.COMM_LOCAL, grp.handle, 0, 2, (2, 1), 5.0)
    try:
        with pytest.raises(gpu.VgsError, match="VGS_E_STATE"):
            t.label_components(np.zeros(4, np.int32), 3)   # rank 0 alone comes back: no collective
        with pytest.raises(gpu.VgsError, match="VGS_E_STATE"):
            t.label_components_result(0, 3)
    finally:
        t.close()
        grp.close()


def test_failures_travel_in_the_status_word(gpu):
    parts = _parts(gpu, (2, 1), n_per=20_000)

    def attempt(call):
        try:
            call()
            return "finished"
        except Exception as ex:  # noqa: BLE001
            return ex

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        n = xyz.shape[0]
        good = np.zeros(n, np.int32)
        bad = good.copy()
        if r == 1:
            bad[[700, 311]] = 3
        res = {}
        res["getter"] = attempt(lambda: t.label_components_result(0, 3))      # after a run, before any call
        res["label"] = attempt(lambda: t.label_components(bad, 3))
        res["n"] = attempt(lambda: t.label_components(good[:-1] if r == 1 else good, 3))
        res["Krange"] = attempt(lambda: t.label_components(good, -1 if r == 1 else 3))
        res["K"] = attempt(lambda: t.label_components(good, 3 + r))
        L = t._L
        res["null"] = L.vgs_tiles_point_label_components(t._h, None if r == 1 else good.ctypes.data_as(C.c_void_p), n, 3, None, None)
        res["after"] = attempt(lambda: t.label_components(good, 3))            # the driver is usable after all of them
        G = gpu._lib.lib()
        st = G.vgs_point_label_components(t._ctx(), good.ctypes.data_as(C.c_void_p), n, 3, None, None)
        res["single"] = (st, G.vgs_last_error_string(t._ctx()).decode())
        return res
    out = _ranks(gpu, (2, 1), _pitch(20_000), parts, body, timeout=120.0)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    E = gpu.VgsError
    for o in out:
        assert isinstance(o["getter"], E) and "VGS_E_STATE" in str(o["getter"])
    assert isinstance(out[1]["label"], E) and "VGS_E_ARG" in str(out[1]["label"]) and "[311] = 3" in str(out[1]["label"]), out[1]["label"]
    for case in ("label", "n", "Krange"):
        assert isinstance(out[1][case], E) and "VGS_E_ARG" in str(out[1][case]), (case, out[1][case])
        assert isinstance(out[0][case], E) and "VGS_E_PEER" in str(out[0][case]) and "rank 1" in str(out[0][case]), (case, out[0][case])
    assert out[1]["null"] == gpu._lib.VGS_E_ARG and out[0]["null"] == gpu._lib.VGS_E_PEER
    for o in out:
        assert isinstance(o["K"], E) and "VGS_E_ARG" in str(o["K"]) and "rank 1 passed K = 4" in str(o["K"]), o["K"]
        assert o["after"] == "finished", o["after"]
        assert o["single"][0] == gpu._lib.VGS_E_STATE and "tile context" in o["single"][1] and "across the ranks" in o["single"][1]


def test_an_injected_failure_takes_the_peer_out(gpu, monkeypatch):
    monkeypatch.setenv("VGS_TILES_FAIL_RANK", "1")
    monkeypatch.setenv("VGS_TILES_FAIL_AT", "components")
    parts = _parts(gpu, (2, 1), n_per=20_000)

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        t.describe_labels(np.zeros(xyz.shape[0], np.int32), 2)     # another phase: not touched
        t.label_components(np.zeros(xyz.shape[0], np.int32), 2)
        return "finished"
    out = _ranks(gpu, (2, 1), _pitch(20_000), parts, body, timeout=120.0)
    assert isinstance(out[1], gpu.VgsError) and "VGS_E_STATE" in str(out[1]) and "components" in str(out[1]), out[1]
    assert isinstance(out[0], gpu.VgsError) and "VGS_E_PEER" in str(out[0]) and "rank 1" in str(out[0]), out[0]


# ---------------------------------------------------------------- 7. the front end
def test_tiles_run_front_end_writes_the_part_tables(gpu, tmp_path):
    tiles = (2, 1)
    parts = _parts(gpu, tiles, n_per=N_PER)
    off = _offsets(parts)
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    n_classes = 5
    cls = [np.ascontiguousarray(((off[r] + np.arange(p.shape[0])) // 1000 % (n_classes + 1) - 1).astype(np.int32)) for r, p in enumerate(parts)]
    outs = {}
    for which in ("refined", "classes"):
        prefix = str(tmp_path / which)
        for r, p in enumerate(parts):
            np.ascontiguousarray(p, dtype=np.float32).tofile(f"{prefix}.{r}.f32")
            cls[r].tofile(f"{prefix}.{r}.classes.i32")
        csv = str(tmp_path / f"{which}.csv")
        opts = ["--refine", "--refined-components", csv] if which == "refined" else ["--class-components", csv, "--classes", str(n_classes)]
        text = subprocess.check_output([EXE, "--emulate", "2x1", "--pitch", repr(float(_pitch(N_PER))), "--voxel", "0.1", *opts, "--component-ids", prefix],
                                       text=True, timeout=300)
        outs[which] = (prefix, csv, int(text.strip().splitlines()[0].split()[1]))

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        _, k = t.point_labels()
        t.refine_labels()
        fine = t.refined_labels().copy()
        return dict(kept=k, refined=t.label_components(fine, k), classes=t.label_components(cls[r], n_classes))
    out = _ranks(gpu, tiles, _pitch(N_PER), parts, body)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    for which, (prefix, csv, kept) in outs.items():
        assert kept == out[0]["kept"]
        c = out[0][which]
        for r in range(2):
            assert np.array_equal(np.fromfile(f"{prefix}.{r}.parts.i32", dtype=np.int32), out[r][which]["part_of_point"]), (which, r)
        with open(csv) as f:
            assert f.readline().strip() == "part,label,n_points,n_nodes,first_code,largest"
        rows = np.loadtxt(csv, delimiter=",", skiprows=1, dtype=np.uint64, ndmin=2)
        assert rows.shape == (c["n_parts"], 6) and np.array_equal(rows[:, 0], np.arange(c["n_parts"], dtype=np.uint64))
        assert np.array_equal(rows[:, 1].astype(np.int32), c["part_label"]) and np.array_equal(rows[:, 2].astype(np.int64), c["part_points"])
        assert np.array_equal(rows[:, 3].astype(np.int32), c["part_nodes"]) and np.array_equal(rows[:, 4], c["part_first_code"])
        largest = np.zeros(c["n_parts"], np.uint64)
        largest[c["label_largest"][c["label_largest"] >= 0]] = 1
        assert np.array_equal(rows[:, 5], largest)
