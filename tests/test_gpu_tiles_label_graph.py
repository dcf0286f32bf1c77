"""Adjacency graph of any per-point labelling across the ranks of the native tiled driver (vgs_tiles_point_label_graph,
include/vgs_tiles.h), ranks as threads of this process over LocalGroup on one GPU.  Every rank hands in the labels of its own points; band
records (code, label) and partial edge tables cross, no point and no label of a point.

The oracle is ONE plain Engine on np.concatenate(parts) -- rank order, the order the shared grid is chained in -- and its label_graph(),
which tests/test_gpu_label_graph.py holds to tests/label_graph_ref.py.  seg_ab, n_shared, n_pairs, n_finite, nodes_ab, w_min and w_max are
compared by bytes; w_sum is held to helpers.check_graph's bar |got - ref| <= 1e-10 |ref| (the ranks' partial sums are added in rank
order), and by bytes with one rank.

Designed scenes are built on the voxel lattice through the origin (voxel_size 0.1; the first point of rank 0, on a lattice corner, fixes
the octree's first box) and split by region; every case asserts a precondition on the plain engine so that it cannot pass vacuously."""
import ctypes as C

import numpy as np
import pytest

from label_refine_ref import floor_and_wall
from label_refine_scenes import GROUP5, WALL, _voxel_points
from segment_scenes import GROUP
from test_gpu_tiles_label_components import ANCHOR, LAYOUTS, N_PER, PRUNED5, _cells, _engine, _split, _voxel_id, _with_anchor
from test_gpu_tiles_point_label_tables import _mixed_labels, _offsets
from test_gpu_tiles_segdesc import _parts, _pitch, _ranks

pytestmark = pytest.mark.gpu
EXACT = ("seg_ab", "n_shared", "n_pairs", "n_finite", "nodes_ab", "w_min", "w_max")
FIELDS = EXACT + ("w_sum",)
# the layouts' two kinds of stored rows: pruned to used neighbours (the default cut threshold) and keeping unused neighbours (no weight is
# cut: every connected group one segment; graph_size 0.25 keeps a neighbourhood below the cut's limit of equal weights); voxels of at
# most five points unused in both
ROWS = {"pruned": dict(voxel_size=0.1, points_min=5), "keep_unused": dict(voxel_size=0.1, graph_size=0.25, points_min=5, cut_thred=100.0)}


# ---------------------------------------------------------------- helpers
def _bytes_equal(a, b, fields=FIELDS):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in fields)


def _assert_table(got, want, what=""):
    """the tiled table against the plain engine's: bytes, w_sum within check_graph's bar"""
    assert got["n_edges"] == want["n_edges"], (what, got["n_edges"], want["n_edges"], got["seg_ab"], want["seg_ab"])
    for k in EXACT:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])
    assert got["w_sum"].dtype == want["w_sum"].dtype
    assert (np.abs(got["w_sum"] - want["w_sum"]) <= 1e-10 * np.abs(want["w_sum"])).all(), (what, got["w_sum"], want["w_sum"])
    assert got["n_skipped"] == want["n_skipped"], (what, got["n_skipped"], want["n_skipped"])


def _body(labs, K):
    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        g = t.label_graph(labs[r], K)
        return dict(g=g, pay=t.label_graph_payload(), times=t.label_graph_times())
    return body


def _against_engine(eng, labs, K, out, what=""):
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    want = eng.label_graph(np.concatenate(labs), K)
    for o in out[1:]:
        assert _bytes_equal(o["g"], out[0]["g"]) and o["g"]["n_skipped"] == out[0]["g"]["n_skipped"]      # every rank: the same bytes
    _assert_table(out[0]["g"], want, what)
    return want


def _designed(gpu, xyz, lab, K, tiles, center, kw):
    parts, labs = _split(xyz, lab, tiles, center)
    assert all(p.shape[0] > 0 for p in parts) and np.array_equal(parts[0][0], ANCHOR[0].astype(np.float32))
    out = _ranks(gpu, tiles, 4.0, parts, _body(labs, K), center=center, params=gpu.default_params(2, **kw), timeout=120.0)
    eng = _engine(gpu, np.concatenate(parts), kw)
    want = _against_engine(eng, labs, K, out)
    return out, want, eng, parts, labs


def _rank_of(xyz, tiles, center):
    """the rank _split gives every point"""
    x, y = xyz[:, 0].astype(np.float32).astype(np.float64), xyz[:, 1].astype(np.float32).astype(np.float64)
    i = (x >= center[0]).astype(np.int64) if tiles[0] == 2 else np.zeros(x.size, np.int64)
    j = (y >= center[1]).astype(np.int64) if tiles[1] == 2 else np.zeros(x.size, np.int64)
    return j * tiles[0] + i


# ---------------------------------------------------------------- 1. two labels meeting at the border
def test_two_labels_meet_at_the_border(gpu):
    rng = np.random.default_rng(1)
    xyz, lab = _with_anchor(_cells(rng, [(i, 2, 2) for i in range(10, 30)]), np.repeat((np.arange(10, 30) >= 20).astype(np.int64), 12))
    out, want, _, _, _ = _designed(gpu, xyz, lab, 2, (2, 1), (2.0, 0.0), GROUP)
    assert want["seg_ab"].tolist() == [[0, 1]] and want["n_shared"].tolist() == [0]
    # graph_size 0.5: four or five voxels a side reach across the border
    assert 10 <= want["n_pairs"][0] <= 15 and want["nodes_ab"][0, 0] == want["nodes_ab"][0, 1] >= 4 and want["n_finite"][0] <= want["n_pairs"][0]
    assert out[0]["g"]["n_pairs"].tolist() == want["n_pairs"].tolist() and out[0]["g"]["nodes_ab"].tolist() == want["nodes_ab"].tolist()
    for o in out:
        assert o["pay"]["band_records"] > 0 and o["pay"]["foreign_hits"] > 0 and o["pay"]["own_edges"] == 1 and o["pay"]["bytes_sent"] > 0
        assert set(o["times"]) == {"own", "exchange1", "table", "exchange2", "fold", "total"} and o["times"]["total"] > 0


# ---------------------------------------------------------------- 2. a voxel cut by the border (x = 2.05)
@pytest.mark.parametrize("same", [False, True], ids=["two_labels", "same_label"])
def test_voxel_cut_by_the_border(gpu, same):
    """(a) the two ranks' points in voxel 20 carry different labels: one shared node, counted once; (b) both carry label 0, beside the
    label-1 voxels 21 and 22: the vertex (0, voxel 20), published by both ranks, is one vertex"""
    rng = np.random.default_rng(3)
    pts = _cells(rng, [(i, 2, 2) for i in range(18, 23)], n=40)
    x = pts[:, 0].astype(np.float32).astype(np.float64)
    lab = (x >= 2.1).astype(np.int64) if same else (x >= 2.05).astype(np.int64)
    xyz, lab = _with_anchor(pts, lab)
    out, want, eng, parts, labs = _designed(gpu, xyz, lab, 2, (2, 1), (2.05, 0.0), GROUP)
    cut = [int(((np.floor(p[:, 0] / np.float32(0.1)) == 20) & (p[:, 1] > 0.15)).sum()) for p in parts]
    assert min(cut) > 0 and sum(cut) == 40, cut                                            # the voxel holds points of both ranks
    assert want["seg_ab"].tolist() == [[0, 1]]
    if same:
        # vertices of label 0 at 18, 19, 20, of label 1 at 21, 22 (graph_size 0.5: all within reach): 3 x 2 contacts
        assert want["n_shared"].tolist() == [0] and want["n_pairs"].tolist() == [6] and want["nodes_ab"].tolist() == [[3, 2]]
        assert all(int((l == 0).sum()) > 0 for l in labs)                                  # label 0 on both ranks
    else:
        # label 0 at 18, 19, 20, label 1 at 20, 21, 22: 3 x 3 pairs less the shared voxel with itself
        assert want["n_shared"].tolist() == [1] and want["n_pairs"].tolist() == [8] and want["nodes_ab"].tolist() == [[3, 3]]
    assert all(o["pay"]["foreign_hits"] > 0 for o in out)


# ---------------------------------------------------------------- 3. pruned rows: a used voxel beside an unused voxel of the other rank
@pytest.mark.parametrize("case", ["a_unused_on_rank_1", "b_second_used_neighbour", "c_mirror"])
def test_used_voxel_beside_an_unused_voxel_of_the_other_rank(gpu, case):
    """rows pruned to used neighbours: the stored row of the used voxel u (label 0) lacks the unused voxel x (three points, label 1) across
    the border; the contact is counted from the full row built for x, on x's owner, and the proxy record that counts u in nodes_ab
    belongs on u's owner"""
    rng = np.random.default_rng(4)
    u, x = ((19, 2, 2), (20, 2, 2)) if case != "c_mirror" else ((20, 2, 2), (19, 2, 2))
    cells = [_voxel_points(rng, u, 30), _voxel_points(rng, x, 3)]
    lab = [np.zeros(30), np.ones(3)]
    if case == "b_second_used_neighbour":
        cells.append(_voxel_points(rng, (18, 2, 2), 30))      # used, label 1, on u's rank
        lab.append(np.ones(30))
    xyz, lab = _with_anchor(np.concatenate(cells), np.concatenate(lab))
    out, want, eng, parts, labs = _designed(gpu, xyz, lab, 2, (2, 1), (2.0, 0.0), PRUNED5)
    vu, vx = _voxel_id(eng, u), _voxel_id(eng, x)
    used = eng.attributes()["used"]
    assert used[vu] and not used[vx]
    off, idx = eng.lists("adjacency")
    assert vx in idx[off[vu]:off[vu + 1]] and vu in idx[off[vx]:off[vx + 1]]
    assert vx not in eng.local_weights(vu)[0].tolist() and vu in eng.local_weights(vu)[0].tolist()   # the stored row is pruned
    assert int((labs[1 if case != "c_mirror" else 0] == 1).sum()) == 3                      # x's points are the other rank's
    assert want["seg_ab"].tolist() == [[0, 1]] and want["n_shared"].tolist() == [0]
    if case == "b_second_used_neighbour":
        assert want["n_pairs"].tolist() == [2] and want["nodes_ab"].tolist() == [[1, 2]]      # u once; a proxy on the wrong rank gives 2
    else:
        assert want["n_pairs"].tolist() == [1] and want["n_finite"].tolist() == [0] and want["nodes_ab"].tolist() == [[1, 1]]
        assert np.isnan(out[0]["g"]["w_min"]).all() and np.isnan(out[0]["g"]["w_max"]).all()


# ---------------------------------------------------------------- 4. 2x2 corner (borders x = 2.05 and y = 2.05)
def test_four_labels_meet_at_the_corner(gpu):
    """every point carries the number of its rank; the voxel (20, 20, 2) holds points of all four ranks, the voxels of row and column 20
    points of two: every pair's shared nodes and contacts are counted once"""
    rng = np.random.default_rng(8)
    cells = [(i, j, 2) for i in range(18, 23) for j in range(18, 23) if (i, j) != (20, 20)]
    quad = np.array([[2.0 + 0.01 + 0.03 * a + 0.05 * sx, 2.0 + 0.01 + 0.03 * b + 0.05 * sy, 0.25] for sx in (0, 1) for sy in (0, 1) for a in (0, 1) for b in (0, 1)])
    pts = np.concatenate([_cells(rng, cells, n=16), quad])
    tiles, center = (2, 2), (2.05, 2.05)
    xyz, lab = _with_anchor(pts, _rank_of(pts, tiles, center))
    out, want, eng, parts, labs = _designed(gpu, xyz, lab, 4, tiles, center, GROUP5)
    assert all(set(l.tolist()) - {-1} == {r} for r, l in enumerate(labs))                   # one label per rank
    corner = [int(((np.floor(p[:, 0] / np.float32(0.1)) == 20) & (np.floor(p[:, 1] / np.float32(0.1)) == 20)).sum()) for p in parts]
    assert corner == [4, 4, 4, 4], corner                                                  # the corner voxel: four points of every rank
    assert want["seg_ab"].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    # ranks 0 | 1 share the voxels (20, 18 .. 20), 2 | 3 the voxels (20, 20 .. 22), 0 | 2 and 1 | 3 those of row 20 alike, the diagonal
    # pairs the corner voxel only
    assert want["n_shared"].tolist() == [3, 3, 1, 1, 3, 3] and (want["n_pairs"] > 0).all()
    assert all(o["pay"]["foreign_hits"] > 0 and o["pay"]["own_edges"] > 0 for o in out)


# ---------------------------------------------------------------- 5. rows above 64 entries at the border
def test_rows_above_64_entries_at_the_border(gpu):
    """the dense cube of test_gpu_label_graph.py (graph_size 0.7), cut by the border x = 0.65"""
    kw = dict(voxel_size=0.1, graph_size=0.7, points_min=7, voxels_min=0)
    xyz = np.random.default_rng(12).uniform(0.0, 1.3, size=(12_000, 3)).astype(np.float32)
    octant = ((xyz[:, 0] > 0.65).astype(np.int32) + 2 * (xyz[:, 1] > 0.65) + 4 * (xyz[:, 2] > 0.65)).astype(np.int32)
    octant[::7] = -1
    parts, labs = _split(xyz, octant, (2, 1), (0.65, 0.0))
    out = _ranks(gpu, (2, 1), 4.0, parts, _body(labs, 8), center=(0.65, 0.0), params=gpu.default_params(2, **kw), timeout=120.0)
    eng = _engine(gpu, np.concatenate(parts), kw)
    used = eng.attributes()["used"].astype(bool)
    stored = max(eng.local_weights(int(v))[0].size for v in np.nonzero(used)[0][::20])
    assert used.sum() > 64 and (~used).any() and stored > 64
    want = _against_engine(eng, labs, 8, out)
    assert want["n_edges"] == 28 and (want["n_shared"] > 0).any() and (want["n_finite"] > 0).all()


# ---------------------------------------------------------------- 6. the engine's own labels
def test_own_labels_give_the_tiled_segment_graph(gpu):
    """floor and wall under WALL, the floor cut by the border y = 2.06"""
    xyz = floor_and_wall()[0]
    tiles, center = (1, 2), (0.0, 2.06)
    kw = WALL
    y = xyz[:, 1].astype(np.float64)
    parts = [np.ascontiguousarray(xyz[y < center[1]]), np.ascontiguousarray(xyz[y >= center[1]])]
    eng = _engine(gpu, np.concatenate(parts), kw)
    kept = eng.counts()["kept"]
    want, seg = eng.label_graph(eng.point_labels(), kept), eng.segment_graph()
    assert kept >= 2 and want["n_edges"] >= 1 and want["n_finite"].sum() > 0 and (want["n_shared"] == 0).all()
    for k in ("seg_ab", "n_pairs", "n_finite", "nodes_ab", "w_min", "w_max"):
        assert want[k].tobytes() == seg[k].tobytes(), k                                     # the precondition, on the plain engine

    def body(r, t, p):
        t.set_points(p)
        t.run()
        pl, k = t.point_labels()
        return dict(kept=k, g=t.label_graph(pl, k), seg=t.segment_graph())
    out = _ranks(gpu, tiles, 4.0, parts, body, center=center, params=gpu.default_params(2, **kw), timeout=120.0)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    for o in out:
        g, s = o["g"], o["seg"]
        assert o["kept"] == kept and (g["n_shared"] == 0).all() and g["n_edges"] == s["seg_ab"].shape[0] >= 1
        for k in ("seg_ab", "n_pairs", "n_finite", "nodes_ab", "w_min", "w_max"):
            assert g[k].tobytes() == s[k].tobytes(), k
        assert (np.abs(g["w_sum"] - s["w_sum"]) <= 1e-10 * np.abs(s["w_sum"])).all()


# ---------------------------------------------------------------- 7. refined and mixed labels on the urban layouts
@pytest.mark.parametrize("rows", sorted(ROWS))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_layouts_match_one_engine_over_the_gathered_points(gpu, layout, rows):
    tiles, shift = LAYOUTS[layout]
    kw = ROWS[rows]
    parts = _parts(gpu, tiles, N_PER, shift)
    bad = np.array([[np.nan, 1.0, 1.0]], np.float32)
    parts = [np.concatenate([p, bad]) for p in parts]   # one point per rank outside the octree, labelled below
    off = _offsets(parts)

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        pl, kept = t.point_labels()
        t.refine_labels()
        fine = t.refined_labels().copy()
        cases = dict(own=(pl, kept), refined=(fine, kept), mixed=(_mixed_labels(pl, off[r], 1), 2 * kept + 3))
        return {name: dict(lab=lab, K=K, g=t.label_graph(lab, K)) for name, (lab, K) in cases.items()}
    center = tuple(shift[:2]) if shift else (0.0, 0.0)
    out = _ranks(gpu, tiles, _pitch(N_PER), parts, body, center=center, params=gpu.default_params(2, **kw))
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    eng = _engine(gpu, np.concatenate(parts), kw)
    inert = not bool((~eng.attributes()["used"].astype(bool)).any()) or _stored_rows_pruned(eng)
    assert inert == (rows == "pruned")
    for name in ("own", "refined", "mixed"):
        K = out[0][name]["K"]
        assert all(o[name]["K"] == K for o in out)
        want = _against_engine(eng, [o[name]["lab"] for o in out], K, [dict(g=o[name]["g"]) for o in out], (layout, rows, name))
        print(layout, rows, name, K, want["n_edges"], int(want["n_pairs"].sum()), int(want["n_shared"].sum()), want["n_skipped"])
    assert out[0]["mixed"]["g"]["n_edges"] > 0 and out[0]["mixed"]["g"]["n_shared"].sum() > 0
    assert out[0]["mixed"]["g"]["n_skipped"] == len(parts)                                   # the NaN points


def _stored_rows_pruned(eng):
    """a used voxel with an unused neighbour whose stored row (local_weights) lacks every unused voxel"""
    used = eng.attributes()["used"].astype(bool)
    off, idx = eng.lists("adjacency")
    has_unused = np.add.reduceat((~used[idx]).astype(np.int64), off[:-1]) > 0
    v = np.nonzero(used & has_unused)[0]
    assert v.size > 0
    ids, _ = eng.local_weights(int(v[0]))
    return not bool((~used[ids]).any())


# ---------------------------------------------------------------- 8. one rank
def test_one_rank_equals_a_plain_engine_byte_for_byte(gpu):
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
        t.refine_labels()
        fine = t.refined_labels().copy()
        eng = _engine(gpu, xyz, dict(voxel_size=0.1))
        for lab, K in ((_mixed_labels(pl, 0, 0), 2 * kept + 3), (fine, kept)):
            before = dict(calls)
            got = t.label_graph(lab, K)
            # two all_gather_varlen: the sizes and the padded payload each
            assert (calls["ag"] - before["ag"], calls["bc"] - before["bc"]) == (4, 0), (before, calls)
            want = eng.label_graph(lab, K)
            assert _bytes_equal(got, want) and got["n_edges"] == want["n_edges"] and got["n_skipped"] == want["n_skipped"]
            pay = t.label_graph_payload()
            assert pay == dict(band_records=0, foreign_hits=0, own_edges=got["n_edges"], bytes_sent=16 * 2 + 56 * (1 + got["n_edges"]))
        assert t.label_graph(_mixed_labels(pl, 0, 0), 2 * kept + 3)["n_edges"] > 0
    finally:
        t.close()


# ---------------------------------------------------------------- 9. the contract
def test_determinism_input_forms_and_neighbouring_calls(gpu):
    import torch
    tiles = (2, 1)
    parts = _parts(gpu, tiles, N_PER)
    off = _offsets(parts)

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        pl, kept = t.point_labels()
        lab, K = _mixed_labels(pl, off[r], 0), 2 * kept + 3
        n = xyz.shape[0]
        first = t.label_graph(lab, K)
        second = t.label_graph(lab, K)
        dev = t.label_graph(torch.as_tensor(lab, device=f"cuda:{t.params.device}"), K)
        getter = t.label_graph_result(first["n_edges"])
        cc = t.label_components(lab, K)                      # the parts pass overwrites the graph's vertex arrays ...
        third = t.label_graph(lab, K)                        # ... and the graph the parts pass's, whose result it drops
        try:
            t.label_components_result(cc["n_parts"], K)
            dropped = False
        except Exception as ex:  # noqa: BLE001
            dropped = "VGS_E_STATE" in str(ex)
        cc2 = t.label_components(lab, K)
        cc_kept = t.label_components_result(cc2["n_parts"], K)
        kept_graph = t.label_graph_result(third["n_edges"])   # the graph's table outlives a parts call
        only = np.where(np.arange(n) % 3 == 0, 0, -1).astype(np.int32) if r == 1 else np.full(n, -1, np.int32)
        empty = dict(k1=t.label_graph(np.zeros(n, np.int32), 1), k0=t.label_graph(np.full(n, -1, np.int32), 0),
                     one_rank_only=t.label_graph(only, 2), none=t.label_graph(np.full(n, -7, np.int32), 4))
        own = t.own_point_label_band(lab, K)
        return dict(first=first, second=second, dev=dev, getter=getter, third=third, kept_graph=kept_graph, dropped=dropped, empty=empty, own=own, K=K,
                    cc_same=all(cc[k].tobytes() == cc2[k].tobytes() == cc_kept[k].tobytes() for k in ("part_of_point", "part_label", "part_points", "part_nodes")))
    out = _ranks(gpu, tiles, _pitch(N_PER), parts, body)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    for o in out:
        assert o["first"]["n_edges"] > 0 and o["cc_same"] and o["dropped"]
        for other in ("second", "dev", "getter", "third", "kept_graph"):
            assert _bytes_equal(o[other], o["first"]), other
        for name, g in o["empty"].items():
            assert g["n_edges"] == 0 and all(g[k].shape[0] == 0 for k in FIELDS), name
        assert o["own"]["band_code"].size == o["own"]["band_label"].size > 0
    assert _bytes_equal(out[0]["first"], out[1]["first"])


def test_own_records_folded_give_the_table(gpu):
    """the C steps by hand: every rank's band, the other rank's records, the partial tables through fold_label_edges"""
    import threading
    from vgs_svgs_segmentation_amd import tiles_native as tn
    tiles = (2, 1)
    parts = _parts(gpu, tiles, N_PER)
    off = _offsets(parts)
    sync = threading.Barrier(2)
    shared = [None, None]

    def body(r, t, xyz):
        try:
            t.set_points(xyz)
            t.run()
            pl, kept = t.point_labels()
            lab, K = _mixed_labels(pl, off[r], 0), 2 * kept + 3
            table = t.label_graph(lab, K)
            shared[r] = t.own_point_label_band(lab, K)
            sync.wait(60)
            o = shared[1 - r]
            part = t.own_point_label_graph(o["band_code"], o["band_label"])
            with pytest.raises(gpu.VgsError, match="VGS_E_STATE"):
                t.link_point_label_parts(o["band_code"], o["band_label"], np.zeros(o["band_label"].size, np.int32), np.zeros(o["band_label"].size, np.int32))
            return dict(table=table, part=part, K=K)
        except Exception:
            sync.abort()
            raise
    out = _ranks(gpu, tiles, _pitch(N_PER), parts, body)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    folded = tn.fold_label_edges([o["part"] for o in out], out[0]["K"])
    assert folded["n_edges"] == out[0]["table"]["n_edges"] > 0 and _bytes_equal(folded, out[0]["table"])
    assert all(o["part"]["n_edges"] > 0 for o in out)


def test_before_a_run_and_before_a_call(gpu):
    from vgs_svgs_segmentation_amd import tiles_native as tn
    grp = tn.LocalGroup(2)
    t = tn.NativeTiles(gpu.default_params(2, voxel_size=0.1), tn.COMM_LOCAL, grp.handle, 0, 2, (2, 1), 5.0)
    try:
        with pytest.raises(gpu.VgsError, match="VGS_E_STATE"):
            t.label_graph(np.zeros(4, np.int32), 3)   # rank 0 alone comes back: no collective
        with pytest.raises(gpu.VgsError, match="VGS_E_STATE"):
            t.label_graph_result(0)
        with pytest.raises(gpu.VgsError, match="VGS_E_STATE"):
            t.own_point_label_band(np.zeros(4, np.int32), 3)
    finally:
        t.close()
        grp.close()
    eng = gpu.Engine(gpu.default_params(2, voxel_size=0.1))     # a plain context
    eng.set_points(np.random.default_rng(0).uniform(0, 1, (2000, 3)).astype(np.float32))
    eng.run()
    G = gpu._lib.lib()
    st = G.vgs_own_point_label_band(eng._h, np.zeros(2000, np.int32).ctypes.data_as(C.c_void_p), 2000, 2, None, None)
    assert st == gpu._lib.VGS_E_STATE and "tile context" in G.vgs_last_error_string(eng._h).decode()


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
        good = (np.arange(n) % 3).astype(np.int32)
        bad = good.copy()
        if r == 1:
            bad[[700, 311]] = 3
        res = {}
        res["getter"] = attempt(lambda: t.label_graph_result(0))               # after a run, before any call
        res["label"] = attempt(lambda: t.label_graph(bad, 3))
        res["n"] = attempt(lambda: t.label_graph(good[:-1] if r == 1 else good, 3))
        res["K"] = attempt(lambda: t.label_graph(good, 3 + r))
        res["after"] = attempt(lambda: t.label_graph(good, 3))                  # the driver is usable after all of them
        G = gpu._lib.lib()
        st = G.vgs_point_label_graph(t._ctx(), good.ctypes.data_as(C.c_void_p), n, 3, None, None)
        res["single"] = (st, G.vgs_last_error_string(t._ctx()).decode())
        return res
    out = _ranks(gpu, (2, 1), _pitch(20_000), parts, body, timeout=120.0)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    E = gpu.VgsError
    for o in out:
        assert isinstance(o["getter"], E) and "VGS_E_STATE" in str(o["getter"])
    assert "[311] = 3" in str(out[1]["label"]), out[1]["label"]
    for case in ("label", "n"):
        assert isinstance(out[1][case], E) and "VGS_E_ARG" in str(out[1][case]), (case, out[1][case])
        assert isinstance(out[0][case], E) and "VGS_E_PEER" in str(out[0][case]) and "rank 1" in str(out[0][case]), (case, out[0][case])
    for o in out:
        assert isinstance(o["K"], E) and "VGS_E_ARG" in str(o["K"]) and "rank 1 passed K = 4" in str(o["K"]), o["K"]
        assert o["after"] == "finished", o["after"]
        assert o["single"][0] == gpu._lib.VGS_E_STATE and "tile context" in o["single"][1] and "across the ranks" in o["single"][1]
        assert "not computed" in o["single"][1] and "vgs_tiles_point_label_graph" in o["single"][1]


def test_an_injected_failure_takes_the_peer_out_and_the_next_call_works(gpu, monkeypatch):
    monkeypatch.setenv("VGS_TILES_FAIL_RANK", "1")
    monkeypatch.setenv("VGS_TILES_FAIL_AT", "label_graph")
    parts = _parts(gpu, (2, 1), n_per=20_000)

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        lab = (np.arange(xyz.shape[0]) % 2).astype(np.int32)
        t.label_components(lab, 2)                                  # another phase: not touched
        try:
            t.label_graph(lab, 2)
            first = "finished"
        except Exception as ex:  # noqa: BLE001
            first = ex
        # the injection strikes every call of its phase; the next collective of another phase works on both ranks
        return dict(first=first, other=t.label_components(lab, 2)["n_parts"])
    out = _ranks(gpu, (2, 1), _pitch(20_000), parts, body, timeout=120.0)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    assert isinstance(out[1]["first"], gpu.VgsError) and "VGS_E_STATE" in str(out[1]["first"]) and "label_graph" in str(out[1]["first"]), out[1]["first"]
    assert isinstance(out[0]["first"], gpu.VgsError) and "VGS_E_PEER" in str(out[0]["first"]) and "rank 1" in str(out[0]["first"]), out[0]["first"]
    assert out[0]["other"] == out[1]["other"] > 0


# ---------------------------------------------------------------- 10. the front end
def test_tiles_run_front_end_writes_the_graph_tables(gpu, tmp_path):
    import os
    import subprocess
    from test_cpp_label_graph import _same as _same_csv
    from test_gpu_tiles_label_components import CSRC, EXE
    tiles = (2, 1)
    parts = _parts(gpu, tiles, n_per=N_PER)
    off = _offsets(parts)
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    n_classes = 5
    cls = [np.ascontiguousarray(((off[r] + np.arange(p.shape[0])) // 1000 % (n_classes + 1) - 1).astype(np.int32)) for r, p in enumerate(parts)]
    prefix = str(tmp_path / "t")
    for r, p in enumerate(parts):
        np.ascontiguousarray(p, dtype=np.float32).tofile(f"{prefix}.{r}.f32")
        cls[r].tofile(f"{prefix}.{r}.classes.i32")
    r_csv, c_csv = str(tmp_path / "refined.csv"), str(tmp_path / "classes.csv")
    text = subprocess.check_output([EXE, "--emulate", "2x1", "--pitch", repr(float(_pitch(N_PER))), "--voxel", "0.1", "--refine", "--refined-graph", r_csv,
                                    "--class-graph", c_csv, "--classes", str(n_classes), prefix], text=True, timeout=300)
    kept = int(text.strip().splitlines()[0].split()[1])

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        _, k = t.point_labels()
        t.refine_labels()
        fine = t.refined_labels().copy()
        return dict(kept=k, refined=t.label_graph(fine, k), classes=t.label_graph(cls[r], n_classes))
    out = _ranks(gpu, tiles, _pitch(N_PER), parts, body)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    assert kept == out[0]["kept"] and out[0]["classes"]["n_edges"] > 0
    _same_csv(r_csv, out[0]["refined"])
    _same_csv(c_csv, out[0]["classes"])
