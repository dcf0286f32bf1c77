"""The label comparison across the ranks of the native tiled driver (vgs_tiles_compare_labels, include/vgs_tiles.h), ranks as threads of
this process over LocalGroup on one GPU.  Every rank hands in the reference ids of its own points only; only contingency cells cross.  All
comparisons of tables are by bytes against tests/label_compare_ref.py over the gathered points, without a tolerance; only the fp64 ARI of
comparison_scores, a host function of those tables, is held to the rounding bound of its own expression (_ari_bound).
  * 2x1, 2x2 and 4x2 layouts of scenes.tiled_urban_scene, and 2x2 far from the origin, seven labellings made per rank from its own points:
    every rank's tables have the same bytes and equal compare_labels over the concatenated labels and ids; comparison_scores agrees with
    the formulas; each rank's own cells are np.unique over its own pairs, and their concatenation gives the tables on a plain engine;
    a second call, a device tensor and a second run give the same bytes; labels, descriptors, graph and boxes are not touched; the
    payload is 24 + 16 bytes per own cell; the run's exchange counter is what it was;
  * one rank: a plain engine's compare_labels byte for byte, through a counting communicator: one all_gather_varlen per call;
  * a rank without an annotated point among ranks with them;
  * failures: an injected one, a wrong n, a call before a run, the tables before a compare and after a new run, the single-context call
    on a tile context;
  * examples/vgs_tiles_run --segment-matches / --truth-matches writes rank 0's tables."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import label_compare_ref as R
from test_gpu_segment_compare import INT32_MAX, INT32_MIN
from test_gpu_tiles_segdesc import _parts, _pitch, _ranks, _same
from test_gpu_tiles_segfields import LAYOUTS, N_PER

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")
FRAMES = ("principal", "upright")
LABELLINGS = ("blocks", "one_id", "own_id", "zero_and_max", "mixed_negative", "all_negative", "labels")
BLOCK = 1.3          # metres; the tile pitch of these layouts is 3.87 m, no multiple of it, so blocks cross tile borders
_cache = {}


def _refs(r, xyz, labels):
    """name -> int32 reference ids of one rank, from its own points, its rank and its own labels alone"""
    n = xyz.shape[0]
    idx = np.arange(n, dtype=np.int64)
    ix = np.floor(xyz[:, 0].astype(np.float64) / BLOCK).astype(np.int64) % 1000
    iy = np.floor(xyz[:, 1].astype(np.float64) / BLOCK).astype(np.int64) % 1000
    rng = np.random.default_rng(40 + r)
    m = rng.integers(-3, 50, n)
    m[rng.choice(n, max(n // 20, 1), replace=False)] = INT32_MIN
    a = np.full(n, -1, np.int64)
    a[::3] = INT32_MIN
    out = dict(blocks=ix + 1000 * iy, one_id=np.full(n, 5, np.int64), own_id=(r << 20) + idx, zero_and_max=np.where(idx % 2 == 0, 0, INT32_MAX),
               mixed_negative=m, all_negative=a, labels=labels.astype(np.int64))
    return {k: np.ascontiguousarray(v.astype(np.int32)) for k, v in out.items()}


def _collect(r, t, xyz):
    torch = pytest.importorskip("torch")
    t.set_points(xyz)
    t.run()
    labels, kept = t.point_labels()
    refs = _refs(r, xyz, labels)
    d, g = t.segment_descriptors(), t.segment_graph()
    b = {f: t.segment_boxes(f) for f in FRAMES}
    ex0 = t.exchange()["collectives"]
    cmp, pay = {}, {}
    for w in LABELLINGS:
        cmp[w] = t.compare_labels(refs[w])
        pay[w] = t.compare_payload()
    times = t.compare_times()
    ex1 = t.exchange()["collectives"]
    second = all(R.same(t.compare_labels(refs[w]), cmp[w]) for w in ("blocks", "mixed_negative", "own_id"))
    device = all(R.same(t.compare_labels(torch.from_numpy(refs[w]).to("cuda:0")), cmp[w]) for w in ("blocks", "mixed_negative"))
    own = {w: t.own_label_cells(kept, refs[w]) for w in LABELLINGS}          # local: every rank on its own
    own_dev = t.own_label_cells(kept, torch.from_numpy(refs["blocks"]).to("cuda:0"))
    labels_after, _ = t.point_labels()
    untouched = (bool(np.array_equal(labels, labels_after)) and _same(d, t.segment_descriptors()) and _same(g, t.segment_graph()) and
                 all(_same(b[f], t.segment_boxes(f)) for f in FRAMES))
    t.run()
    labels2, kept2 = t.point_labels()
    rerun = bool(np.array_equal(labels, labels2)) and kept2 == kept and all(R.same(t.compare_labels(refs[w]), cmp[w]) for w in ("blocks", "labels"))
    return dict(labels=labels, kept=kept, refs=refs, cmp=cmp, pay=pay, times=times, ex=(ex0, ex1), second=second, device=device, own=own,
                own_dev=own_dev, untouched=untouched, rerun=rerun)


def _layout(gpu, name):
    if name not in _cache:
        tiles, shift = LAYOUTS[name]
        parts = _parts(gpu, tiles, shift=shift)
        out = _ranks(gpu, tiles, _pitch(N_PER), parts, _collect, center=shift[:2] if shift else (0.0, 0.0))
        for r, o in enumerate(out):
            assert not isinstance(o, Exception), (r, o)
        labels = np.concatenate([o["labels"] for o in out])
        kept = out[0]["kept"]
        want = {w: R.compare_labels(labels, np.concatenate([o["refs"][w] for o in out]), kept) for w in LABELLINGS}   # once, shared
        _cache[name] = (parts, out, labels, kept, want)
    return _cache[name]


def _plain(gpu):
    """a segmented plain engine for vgs_label_comparison_from_cells on a context of its own"""
    if "plain" not in _cache:
        eng = gpu.Engine(gpu.default_params(2, voxel_size=0.1))
        eng.set_points(gpu.scenes.urban_scene(20_000))
        eng.run()
        _cache["plain"] = eng
    return _cache["plain"]


def _pairs_of(o, w):
    """np.unique over one rank's own annotated (label, id) pairs: keys (label + 1) << 31 | id and counts"""
    L, g = o["labels"].astype(np.int64), o["refs"][w].astype(np.int64)
    ann = g >= 0
    return np.unique((L[ann] + 1) * (1 << 31) + g[ann], return_counts=True)


def _ari_bound(s):
    """How far comparison_scores' fp64 ARI may lie from the exact rational one, from the roundings of its own expression
    (c - e) / ((a + b) / 2 - e), e = a b / T, with c, a, b = summary[8..10] and T = C(n, 2) (u = 2^-52, twice the unit roundoff, so that
    second-order terms are covered).  c, a and b are integers that a double holds or rounds once (u each); e takes three roundings (the
    product, T, the quotient): |e' - e| <= 3 u e.  Numerator: |num' - num| <= u c + 3 u e + u |num| =: En -- the subtraction cancels, which
    is why a relative bound on the score would not do.  Denominator: |den' - den| <= 2 u (a + b) / 2 + 3 u e + u |den| =: Ed.  The quotient
    adds one rounding, the conversion of the exact value to a double another: |ari' - ari| <= En / |den| + |ari| (Ed / |den| + 2 u)."""
    from fractions import Fraction
    u = Fraction(1, 1 << 52)
    c, a, b, n = int(s[8]), int(s[9]), int(s[10]), int(s[0])
    T = n * (n - 1) // 2
    e = Fraction(a * b, T)
    num, den = c - e, Fraction(a + b, 2) - e
    En, Ed = u * c + 3 * u * e + u * abs(num), u * (a + b) + 3 * u * e + u * abs(den)
    return float(En / abs(den) + abs(num / den) * (Ed / abs(den) + 2 * u))


# ---------------------------------------------------------------- layouts x labellings
@pytest.mark.parametrize("which", LABELLINGS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_tiled_tables_equal_the_gathered_points(gpu, name, which):
    parts, out, labels, kept, want = _layout(gpu, name)
    assert kept > 0 and labels.max() == kept - 1
    for r, o in enumerate(out):
        assert o["kept"] == kept
        assert R.same(o["cmp"][which], want[which]), (r, R.diff(o["cmp"][which], want[which]), o["cmp"][which]["summary"], want[which]["summary"])
    got = out[0]["cmp"][which]
    s = got["summary"]
    assert s[0] + s[1] == labels.size and got["seg_annotated"].shape == (kept,)
    sc, sf = gpu.comparison_scores(got, 0.5), R.scores_formulas(got, 0.5)
    assert sc["matched"] == sf["matched"]
    for k in ("precision", "recall", "f1", "purity", "completeness"):           # one or two divisions of small integers
        assert R.close(sc[k], sf[k]), (k, sc[k], sf[k])
    if sf["ari"] != sf["ari"]:
        assert sc["ari"] != sc["ari"]
    else:
        print(which, "ari", sc["ari"], sf["ari"], abs(sc["ari"] - sf["ari"]), _ari_bound(s))
        assert abs(sc["ari"] - sf["ari"]) <= _ari_bound(s), (sc["ari"], sf["ari"], _ari_bound(s))
    if which == "own_id":
        assert s[4] == s[3] == labels.size and (got["cell_n"] == 1).all() and s[8] == 0
    if which == "zero_and_max":
        assert got["ref_id"].tolist() == [0, INT32_MAX]
    if which == "all_negative":
        assert s.tolist() == [0, labels.size] + [0] * 10 and got["cell_n"].size == 0 and (got["seg_best_ref"] == -1).all()
    if which == "labels":
        # the perfect match: diagonal cells, every kept segment (each has a point) at IoU 1
        assert (got["seg_best_iou"] == 1.0).all() and (got["ref_best_iou"] == 1.0).all()
        assert np.array_equal(got["cell_seg"], got["cell_ref"]) and np.array_equal(got["cell_seg"], np.arange(kept))
        assert s[6] == s[7] == s[0] - s[2] and s[2] == 0 and s[1] == int((labels < 0).sum())


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_layouts_exercise_the_merge(gpu, name):
    """conditions of the inputs, so that no layout passes on a degenerate case: a merged cell, an id and a kept segment with points on two
    ranks each (blocks and one id), computed from the ranks' own cells"""
    parts, out, labels, kept, want = _layout(gpu, name)
    world = len(parts)
    for w in ("blocks", "one_id"):
        keys = [o["own"][w]["cell_seg"].astype(np.int64) * (1 << 31) + o["own"][w]["cell_ref"] for o in out]
        allk, cnt = np.unique(np.concatenate(keys), return_counts=True)
        assert (cnt >= 2).any(), (name, w)                                                  # one pair counted on two ranks
        assert allk.size == want[w]["cell_seg"].size < sum(k.size for k in keys)
        ids = [np.unique(o["own"][w]["cell_ref"]) for o in out]
        assert (np.unique(np.concatenate(ids), return_counts=True)[1] >= 2).any(), (name, w)   # an id on two ranks
    rank_of = np.repeat(np.arange(world), [p.shape[0] for p in parts])
    lab_ranks = np.zeros((kept, world), bool)
    lab_ranks[labels[labels >= 0], rank_of[labels >= 0]] = True
    assert (lab_ranks.sum(axis=1) >= 2).any()                                                # a kept segment on two ranks


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_own_cells_repeats_and_side_effects(gpu, name):
    parts, out, labels, kept, want = _layout(gpu, name)
    eng = _plain(gpu)
    for r, o in enumerate(out):
        assert o["second"] and o["device"] and o["rerun"] and o["untouched"], (r, o["second"], o["device"], o["rerun"], o["untouched"])
        assert o["ex"][0] == o["ex"][1] >= 1                                                 # the run's exchange is not taken again
        assert o["times"]["total"] > 0 and o["times"]["exchange"] >= 0 and o["times"]["own"] >= 0 and o["times"]["tables"] > 0
        for w in LABELLINGS:
            own = o["own"][w]
            key, n = _pairs_of(o, w)
            assert own["cell_seg"].dtype == np.int32 and own["cell_ref"].dtype == np.int32 and own["cell_n"].dtype == np.int64
            assert np.array_equal(own["cell_seg"].astype(np.int64), key // (1 << 31) - 1) and np.array_equal(own["cell_ref"].astype(np.int64), key % (1 << 31)), (r, w)
            assert np.array_equal(own["cell_n"], n) and own["n_unannotated"] == int((o["refs"][w] < 0).sum()), (r, w)
            assert o["pay"][w] == dict(own_cells=key.size, bytes_sent=24 + 16 * key.size), (r, w, o["pay"][w])
        assert all(np.array_equal(o["own_dev"][k], o["own"]["blocks"][k]) for k in ("cell_seg", "cell_ref", "cell_n"))
    for w in LABELLINGS:
        cat = [np.concatenate([o["own"][w][k] for o in out]) for k in ("cell_seg", "cell_ref", "cell_n")]
        got = eng.label_comparison_from_cells(*cat, sum(o["own"][w]["n_unannotated"] for o in out), K=kept)
        assert R.same(got, want[w]), (w, R.diff(got, want[w]))


# ---------------------------------------------------------------- one rank; a rank without annotation
def test_one_rank_equals_a_plain_engine_with_one_exchange_per_call(gpu):
    """1x1 through a communicator that counts: the table is a plain engine's, and a call makes two all-gathers -- the sizes and the padded
    payload of ONE all_gather_varlen -- and no broadcast"""
    from vgs_svgs_segmentation_amd import tiles_native as tn
    xyz = _parts(gpu, (1, 1))[0]
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
        labels, kept = t.point_labels()
        refs = _refs(0, xyz, labels)
        eng = gpu.Engine(gpu.default_params(2, voxel_size=0.1))
        eng.set_points(xyz)
        eng.run()
        assert eng.counts()["kept"] == kept and np.array_equal(eng.point_labels(), labels)
        for w in LABELLINGS:
            before = dict(calls)
            got = t.compare_labels(refs[w])
            assert (calls["ag"] - before["ag"], calls["bc"] - before["bc"]) == (2, 0), (w, before, calls)
            want = eng.compare_labels(refs[w])
            assert R.same(got, want), (w, R.diff(got, want))
    finally:
        t.close()


def test_a_rank_without_an_annotated_point(gpu):
    parts, base, labels, kept, _ = _layout(gpu, "2x1")

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        ref = base[r]["refs"]["blocks"] if r == 0 else np.full(xyz.shape[0], -7, np.int32)
        return ref, t.compare_labels(ref), t.compare_payload()
    out = _ranks(gpu, (2, 1), _pitch(N_PER), parts, body)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    want = R.compare_labels(labels, np.concatenate([o[0] for o in out]), kept)
    assert R.same(out[0][1], want) and R.same(out[1][1], want), R.diff(out[0][1], want)
    assert out[1][2] == dict(own_cells=0, bytes_sent=24) and want["summary"][1] >= parts[1].shape[0] and want["summary"][0] > 0


# ---------------------------------------------------------------- failures
def _status(gpu, x):
    assert isinstance(x, gpu.VgsError), x
    return x.status


def test_a_failing_rank_takes_its_peer_out(gpu, monkeypatch):
    monkeypatch.setenv("VGS_TILES_FAIL_RANK", "1")
    monkeypatch.setenv("VGS_TILES_FAIL_AT", "compare")
    parts = _parts(gpu, (2, 1))

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        t.compare_labels(np.zeros(xyz.shape[0], np.int32))
        return "finished"
    out = _ranks(gpu, (2, 1), _pitch(N_PER), parts, body, timeout=120.0)
    assert _status(gpu, out[1]) == gpu._lib.VGS_E_STATE and "compare" in str(out[1]), out[1]
    assert _status(gpu, out[0]) == gpu._lib.VGS_E_PEER and "rank 1" in str(out[0]), out[0]


@pytest.mark.parametrize("which", ["short", "long", "null"])
def test_a_wrong_n_travels_in_the_status_word(gpu, which):
    """rank 1 passes one id too few, one too many, no array: its own VGS_E_ARG, rank 0 VGS_E_PEER, and nobody is left inside the driver"""
    parts = _parts(gpu, (2, 1))

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        n = xyz.shape[0]
        if r == 1 and which == "null":
            t._ck(t._L.vgs_tiles_compare_labels(t._h, None, n, None, None, None, None))
        else:
            t.compare_labels(np.zeros(n + (0 if r == 0 else -1 if which == "short" else 1), np.int32))
        return "finished"
    out = _ranks(gpu, (2, 1), _pitch(N_PER), parts, body, timeout=120.0)
    assert _status(gpu, out[1]) == gpu._lib.VGS_E_ARG and ("ref is NULL" if which == "null" else "n_own") in str(out[1]), (which, out[1])
    assert _status(gpu, out[0]) == gpu._lib.VGS_E_PEER and "rank 1" in str(out[0]), (which, out[0])


def test_bad_calls_are_refused_without_a_collective(gpu):
    """one rank of two, whose peer never calls: the errors come back, so they are decided locally"""
    from vgs_svgs_segmentation_amd import tiles_native as tn
    grp = tn.LocalGroup(2)
    t = tn.NativeTiles(gpu.default_params(2, voxel_size=0.1), tn.COMM_LOCAL, grp.handle, 0, 2, (2, 1), 5.0)
    try:
        with pytest.raises(gpu.VgsError) as e:
            t.compare_labels(np.zeros(4, np.int32))
        assert e.value.status == gpu._lib.VGS_E_STATE and "vgs_tiles_run first" in str(e.value)
        with pytest.raises(gpu.VgsError) as e:
            t.label_comparison(0, 0, 0)
        assert e.value.status == gpu._lib.VGS_E_STATE
        with pytest.raises(gpu.VgsError) as e:
            t.own_label_cells(0, np.zeros(4, np.int32))
        assert e.value.status == gpu._lib.VGS_E_STATE
    finally:
        t.close()
        grp.close()


def test_tables_need_a_compare_since_the_last_run_and_the_single_context_call_is_still_refused(gpu):
    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        n = xyz.shape[0]
        raw = lambda: t._L.vgs_tiles_get_label_comparison(t._h, *([None] * 14))   # noqa: E731
        st = [raw()]                                                               # a run, no compare yet
        ref = (np.arange(n) % 13).astype(np.int32)
        got = t.compare_labels(ref)
        st.append(raw())
        t.run()
        st.append(raw())                                                           # a new run: gone
        again = t.compare_labels(ref)
        st.append(raw())
        L, h = gpu._lib.lib(), t._ctx()
        m = t.counts()["points"]                                                   # tile + halo: the context's own cloud
        st1 = L.vgs_compare_labels(h, np.zeros(m, np.int32).ctypes.data_as(C.c_void_p), m, None, None, None)
        msg = L.vgs_last_error_string(h)
        t.set_points(xyz)
        st.append(raw())                                                           # new points: gone
        return st, R.same(got, again), st1, msg
    out = _ranks(gpu, (2, 1), _pitch(N_PER), _parts(gpu, (2, 1)), body)
    E = gpu._lib.VGS_E_STATE
    for o in out:
        assert not isinstance(o, Exception), o
        assert o[0] == [E, 0, E, 0, E] and o[1]
        assert o[2] == E and b"tile context" in o[3]


# ---------------------------------------------------------------- front end
def test_tiles_run_front_end_writes_the_matches(gpu, tmp_path):
    parts, base, labels, kept, want = _layout(gpu, "2x2")
    w = want["mixed_negative"]
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    prefix = str(tmp_path / "t")
    for r, p in enumerate(parts):
        np.ascontiguousarray(p, dtype=np.float32).tofile(f"{prefix}.{r}.f32")
        base[r]["refs"]["mixed_negative"].tofile(f"{prefix}.{r}.truth.i32")
    seg_csv, ref_csv = str(tmp_path / "seg.csv"), str(tmp_path / "truth.csv")
    out = subprocess.check_output([EXE, "--emulate", "2x2", "--pitch", repr(float(_pitch(N_PER))), "--voxel", "0.1", "--segment-matches", seg_csv,
                                   "--truth-matches", ref_csv, prefix], text=True, timeout=300)
    assert int(out.strip().splitlines()[-1].split()[1]) == kept
    with open(seg_csv) as f:
        assert f.readline().strip() == "label,n_annotated,n_refs,best_ref,best_n,best_iou"
    rows = np.loadtxt(seg_csv, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    assert rows.shape == (kept, 6) and np.array_equal(rows[:, 0], np.arange(kept))
    for col, name in enumerate(("seg_annotated", "seg_refs", "seg_best_ref", "seg_best_n"), 1):
        assert np.array_equal(rows[:, col].astype(np.int64), w[name]), name
    assert np.array_equal(rows[:, 5], w["seg_best_iou"])                          # %.17g reads back exactly
    with open(ref_csv) as f:
        assert f.readline().strip() == "ref_id,n_points,n_dropped,best_seg,best_n,best_iou"
    rows = np.loadtxt(ref_csv, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    assert rows.shape == (w["ref_id"].size, 6)
    for col, name in enumerate(("ref_id", "ref_points", "ref_dropped", "ref_best_seg", "ref_best_n")):
        assert np.array_equal(rows[:, col].astype(np.int64), w[name]), name
    assert np.array_equal(rows[:, 5], w["ref_best_iou"])
