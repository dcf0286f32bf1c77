"""The comparison tables from a list of contingency cells (vgs_label_comparison_from_cells, include/vgs.h; Engine.label_comparison_from_cells):
the merge of the cells on the device and the tables behind it, alone, on one plain engine, from hand-made cells.  Everything is compared by
bytes against tests/label_compare_ref.py over the points the cells stand for; no tolerance appears.
  * the cells of 1, 2, 3 and 8 random shares of a labelled cloud, concatenated and shuffled: compare_labels over all points, whatever the
    order of the input;
  * n_in = 0, 1, 255, 256, 257 (the workgroup edge); runs of 1, 2, 8 and 300 entries for one pair; a row and an id with more than 64 merged
    cells (the lane-stride loops of the table kernels, fed by the merge);
  * 64-bit counts: 2^31 + 2^31 for one pair, sums checked against Python integers; a total of 2^32 + 1 is refused;
  * ties across shares; ids 0 and INT32_MAX; K = 0; no cell at all;
  * VGS_E_ARG naming the first offending input, and the context still compares afterwards; side effects."""
import ctypes as C

import numpy as np
import pytest

import label_compare_ref as R
from test_gpu_segment_compare import INT32_MAX, INT32_MIN, _engine, _eq, _others

pytestmark = pytest.mark.gpu
_cache = {}


def _eng(gpu):
    """one segmented plain engine with its cloud's labels and an own reference, made once; the tests leave it segmented"""
    if "eng" not in _cache:
        xyz = gpu.scenes.town_scene(60_000)
        eng = _engine(gpu, xyz)
        ref = (np.arange(xyz.shape[0]) % 37 - 2).astype(np.int32)
        _cache["eng"] = (eng, ref, eng.compare_labels(ref))
    return _cache["eng"]


def _cells(labels, ref):
    """np.unique over the annotated (label, id) pairs of some points: cell_seg, cell_ref, cell_n"""
    L, g = np.asarray(labels).astype(np.int64), np.asarray(ref).astype(np.int64)
    ann = g >= 0
    key, n = np.unique((L[ann] + 1) * (1 << 31) + g[ann], return_counts=True)
    return (key // (1 << 31) - 1).astype(np.int32), (key % (1 << 31)).astype(np.int32), n.astype(np.int64)


def _points(seg, ref, n, unann):
    """the points a cell list stands for: labels and ids, `unann` points without annotation behind them"""
    seg, ref, n = np.asarray(seg, np.int64), np.asarray(ref, np.int64), np.asarray(n, np.int64)
    return (np.concatenate([np.repeat(seg, n), np.full(unann, -1, np.int64)]).astype(np.int32),
            np.concatenate([np.repeat(ref, n), np.full(unann, -1, np.int64)]).astype(np.int32))


def _expect(eng, seg, ref, n, unann, K):
    got = eng.label_comparison_from_cells(seg, ref, n, unann, K=K)
    want = R.compare_labels(*_points(seg, ref, n, unann), K)
    assert R.same(got, want), R.diff(got, want)
    return got


def test_shares_of_a_cloud_give_the_tables_of_all_points(gpu):
    eng, _, _ = _eng(gpu)
    rng = np.random.default_rng(11)
    N, K = 5000, 40
    labels = rng.integers(-1, K, N).astype(np.int32)
    ref = rng.integers(-3, 200, N).astype(np.int64)
    ref[rng.choice(N, 50, replace=False)] = INT32_MIN
    ref = ref.astype(np.int32)
    assert (labels == -1).any() and (ref < 0).any()
    want = R.compare_labels(labels, ref, K)
    unann = int((ref < 0).sum())
    for shares in (1, 2, 3, 8):
        share = rng.integers(0, shares, N)
        lists = [_cells(labels[share == s], ref[share == s]) for s in range(shares)]
        seg, rf, n = (np.concatenate([l[j] for l in lists]) for j in range(3))
        assert shares == 1 or seg.size > want["cell_seg"].size          # pairs do repeat across the shares
        for _ in range(2):                                              # the order of the input does not matter
            order = rng.permutation(seg.size)
            got = eng.label_comparison_from_cells(seg[order], rf[order], n[order], unann, K=K)
            assert R.same(got, want), (shares, R.diff(got, want))


@pytest.mark.parametrize("n_in", [0, 1, 255, 256, 257])
def test_input_sizes_around_a_workgroup(gpu, n_in):
    eng, _, _ = _eng(gpu)
    rng = np.random.default_rng(100 + n_in)
    K = 9
    seg, ref, n = rng.integers(-1, K, n_in), rng.integers(0, 30, n_in), rng.integers(1, 6, n_in)
    got = _expect(eng, seg, ref, n, 4, K)
    assert got["summary"][0] == n.sum() and got["summary"][1] == 4
    if n_in == 0:
        assert got["summary"].tolist() == [0, 4] + [0] * 10 and got["cell_seg"].size == 0 and got["ref_id"].size == 0
        assert (got["seg_annotated"].tolist(), got["seg_refs"].tolist(), got["seg_best_ref"].tolist(), got["seg_best_n"].tolist(),
                got["seg_best_iou"].tolist()) == ([0] * K, [0] * K, [-1] * K, [0] * K, [0.0] * K)


@pytest.mark.parametrize("run", [1, 2, 8, 300])
def test_runs_of_one_pair(gpu, run):
    """`run` entries for the pair (3, 9) between other cells: longer than a wavefront and than a workgroup at 300"""
    eng, _, _ = _eng(gpu)
    rng = np.random.default_rng(run)
    seg = np.concatenate([[0, 3, 3, 5, -1], np.full(run, 3)])
    ref = np.concatenate([[9, 8, 10, 9, 9], np.full(run, 9)])
    n = np.concatenate([[2, 1, 4, 3, 2], np.arange(1, run + 1)])
    order = rng.permutation(seg.size)
    got = _expect(eng, seg[order], ref[order], n[order], 0, 6)
    i = np.flatnonzero((got["cell_seg"] == 3) & (got["cell_ref"] == 9))
    assert i.size == 1 and got["cell_n"][i[0]] == run * (run + 1) // 2 and got["cell_seg"].size == 6


def test_a_row_and_an_id_of_more_than_64_merged_cells(gpu):
    eng, _, _ = _eng(gpu)
    rng = np.random.default_rng(5)
    K = 100
    row = (np.full(200, 2), np.tile(np.arange(100), 2), rng.integers(1, 9, 200))                 # segment 2: 100 ids, each pair twice
    col = (np.tile(np.arange(20, 100), 3), np.full(240, 500), rng.integers(1, 9, 240))           # id 500: 80 segments, each pair three times
    seg, ref, n = (np.concatenate([row[j], col[j]]) for j in range(3))
    order = rng.permutation(seg.size)
    got = _expect(eng, seg[order], ref[order], n[order], 1, K)
    assert got["seg_refs"][2] == 100 and got["cell_seg"].size == 180
    assert got["ref_points"][got["ref_id"] == 500][0] == col[2].sum()


def test_counts_beyond_32_bits(gpu):
    """Two cells of 2^31 for one pair: cell_n = 2^32, and the pair sums are C(2^32, 2), held against Python integers.  The total is then at
    the limit of 2^32 already, so a further pair on the same id fits only with one of the two cells smaller: the second case takes 2^31 - 3
    there and gives the other pair the 3.  One more point than 2^32 is refused."""
    eng, _, _ = _eng(gpu)
    lib = gpu._lib
    c2 = lambda a: a * (a - 1) // 2   # noqa: E731
    H = 1 << 31
    got = eng.label_comparison_from_cells([0, 0], [5, 5], [H, H], 7, K=2)
    assert got["cell_n"].tolist() == [1 << 32] and got["cell_n"].dtype == np.int64
    assert got["summary"].tolist() == [1 << 32, 7, 0, 1, 1, 1, 1 << 32, 1 << 32, c2(1 << 32), c2(1 << 32), c2(1 << 32), 0]
    assert got["seg_annotated"].tolist() == [1 << 32, 0] and got["ref_points"].tolist() == [1 << 32]
    assert got["seg_best_iou"].tolist() == [1.0, 0.0] and got["ref_best_iou"].tolist() == [1.0]
    got = eng.label_comparison_from_cells([0, 1, 0], [5, 5, 5], [H, 3, H - 3], 0, K=2)
    a = (1 << 32) - 3
    assert (got["cell_seg"].tolist(), got["cell_ref"].tolist(), got["cell_n"].tolist()) == ([0, 1], [5, 5], [a, 3])
    assert got["summary"][0] == 1 << 32 and got["summary"][8:11].tolist() == [c2(a) + c2(3), c2(a) + c2(3), c2(1 << 32)]
    assert got["ref_points"].tolist() == [1 << 32] and got["ref_best_seg"].tolist() == [0] and got["ref_best_n"].tolist() == [a]
    assert got["ref_best_iou"][0] == float(a) / float(1 << 32) and got["seg_best_iou"].tolist() == [float(a) / float(1 << 32), 3.0 / float(1 << 32)]
    for n in ([H, H, 1], [H, H + 1], [(1 << 62), (1 << 62), (1 << 62), (1 << 62)]):
        with pytest.raises(gpu.VgsError) as e:
            eng.label_comparison_from_cells([0] * len(n), [5] * len(n), n, 0, K=2)
        assert e.value.status == lib.VGS_E_UNSUPPORTED and "2^32" in str(e.value), (n, e.value)
    # n_in itself: refused before anything is read
    one = np.zeros(1, np.int64)
    p = one.ctypes.data_as(C.c_void_p)
    assert eng._L.vgs_label_comparison_from_cells(eng._h, 2, 1 << 31, p, p, p, 0, None, None, None) == lib.VGS_E_UNSUPPORTED
    assert b"2^31" in eng._L.vgs_last_error_string(eng._h)
    _expect(eng, [0], [5], [1], 0, 2)


def test_ties_across_shares(gpu):
    """id 7: c points in segment A from one share and c in segment B from another (A's in two entries); id 3: c points in A.  The lowest
    label wins id 7 and the lowest id wins A: the rule of include/vgs.h, here against the loops of compare_brute."""
    eng, _, _ = _eng(gpu)
    A, B, c, K = 4, 2, 5, 6
    seg, ref, n = [B, A, A, A, 1], [7, 7, 3, 7, 3], [c, 2, c, c - 2, 1]
    got = eng.label_comparison_from_cells(seg, ref, n, 0, K=K)
    want = R.compare_brute(*_points(seg, ref, n, 0), K)
    assert R.same(got, want), R.diff(got, want)
    assert got["ref_best_seg"][got["ref_id"] == 7][0] == min(A, B) and got["seg_best_ref"][A] == 3 and got["seg_best_n"][A] == c


def test_extreme_ids_and_no_segments(gpu):
    eng, _, _ = _eng(gpu)
    got = _expect(eng, [0, 1, 0, -1, 1], [0, INT32_MAX, INT32_MAX, 0, INT32_MAX], [2, 3, 1, 4, 2], 0, 2)
    assert got["ref_id"].tolist() == [0, INT32_MAX]
    k0 = _expect(eng, [-1, -1, -1], [0, INT32_MAX, 0], [2, 3, 1], 5, 0)                            # K = 0: every cell in the -1 row
    assert k0["seg_annotated"].shape == (0,) and k0["summary"][2] == 6 and (k0["ref_best_seg"] == -1).all() and k0["cell_n"].tolist() == [3, 3]
    none = eng.label_comparison_from_cells([], [], [], 17, K=0)
    assert none["summary"].tolist() == [0, 17] + [0] * 10 and all(none[k].size == 0 for k, _ in R.FIELDS if k != "summary")


@pytest.mark.parametrize("bad,word", [((5, 1, 1), "seg 5"), ((-2, 1, 1), "seg -2"), ((0, -1, 1), "ref -1"), ((0, 1, 0), "n 0")])
def test_an_input_that_is_not_a_cell_is_named(gpu, bad, word):
    """seg = K, seg = -2, ref = -1, count = 0 at input 300 of 600, and another bad one behind it: VGS_E_ARG with the first one's index and
    values; no table is left behind, and the context compares as before"""
    eng, _, _ = _eng(gpu)
    rng = np.random.default_rng(3)
    K = 5
    seg, ref, n = rng.integers(-1, K, 600), rng.integers(0, 20, 600), rng.integers(1, 4, 600)
    good = (seg.copy(), ref.copy(), n.copy())
    seg[300], ref[300], n[300] = bad
    seg[450] = K + 3
    with pytest.raises(gpu.VgsError) as e:
        eng.label_comparison_from_cells(seg, ref, n, 0, K=K)
    assert e.value.status == gpu._lib.VGS_E_ARG and "input cell 300 " in str(e.value) and word in str(e.value), e.value
    assert eng._L.vgs_get_label_comparison(eng._h, *([None] * 14)) == gpu._lib.VGS_E_STATE
    _expect(eng, *good, 0, K)


def test_arguments_and_state(gpu):
    lib = gpu._lib
    eng, _, _ = _eng(gpu)
    one = np.ones(1, np.int64)
    p = one.ctypes.data_as(C.c_void_p)
    f = eng._L.vgs_label_comparison_from_cells
    assert f(eng._h, -1, 0, None, None, None, 0, None, None, None) == lib.VGS_E_ARG
    assert f(eng._h, 2, -1, None, None, None, 0, None, None, None) == lib.VGS_E_ARG
    assert f(eng._h, 2, 0, None, None, None, -1, None, None, None) == lib.VGS_E_ARG
    assert f(eng._h, 2, 1, None, p, p, 0, None, None, None) == lib.VGS_E_ARG and b"NULL" in eng._L.vgs_last_error_string(eng._h)
    assert f(eng._h, 2, 0, None, None, None, 3, None, None, None) == lib.VGS_OK                    # every output NULL, no input at all
    fresh = gpu.Engine(gpu.default_params(2))
    with pytest.raises(gpu.VgsError) as e:
        fresh.label_comparison_from_cells([0], [0], [1], 0, K=1)
    assert e.value.status == lib.VGS_E_STATE
    # the own-cell calls are for tile contexts only
    nc = C.c_int64(0)
    r = np.zeros(eng.counts()["points"], np.int32)
    st = eng._L.vgs_own_label_cells(eng._h, eng.counts()["kept"], r.ctypes.data_as(C.c_void_p), r.size, C.byref(nc), None)
    assert st == lib.VGS_E_STATE and b"tile context" in eng._L.vgs_last_error_string(eng._h)
    assert eng._L.vgs_get_own_label_cells(eng._h, None, None, None) == lib.VGS_E_STATE


def test_side_effects(gpu):
    eng, ref, first = _eng(gpu)
    before = _others(eng)
    rng = np.random.default_rng(8)
    K = eng.counts()["kept"]
    seg, rf, n = rng.integers(-1, K, 1000), rng.integers(0, 50, 1000), rng.integers(1, 4, 1000)
    got = _expect(eng, seg, rf, n, 2, K)
    # the tables are the context's last comparison
    again = {name: np.zeros(got[name].shape, dt) for name, dt, _ in gpu.Engine.COMPARE_FIELDS}
    eng._ck(eng._L.vgs_get_label_comparison(eng._h, *(again[name].ctypes.data_as(C.c_void_p) for name, _, _ in gpu.Engine.COMPARE_FIELDS)))
    again["summary"] = got["summary"]
    assert R.same(again, got)
    ptrs = eng.label_comparison_device()
    assert ptrs["cell_n"] and ptrs["ref_id"] and ptrs["seg_annotated"]
    assert _eq(before, _others(eng))                                   # labels, clusters, descriptors, graph, boxes: byte for byte
    assert R.same(eng.compare_labels(ref), first)                      # and the engine's own compare gives what it gave
