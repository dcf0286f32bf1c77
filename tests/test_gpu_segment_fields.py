"""Per-segment statistics of caller-supplied point attributes (vgs_segment_field_stats, vgs_segment_class_histogram; csrc/segfield.hip):
  * integer-valued fields, whose sums are exact in any order: n_valid, mean, var, vmin, vmax equal to tests/segment_fields_ref.py evaluated
    with the engine's own anchor, by value and without a tolerance -- for 1, 3, 5 and 64 channels, a padded row stride and a device tensor;
  * the anchor contract; identities against the descriptor table (xyz as the field) and for a per-segment constant;
  * general floats against math.fsum within the worst-case bound of a summation of n terms; NaN and +-inf;
  * the class histogram against the restatement, ties, all-outside segments, the device variant;
  * determinism, no side effects on the other getters, the state and argument contract.
Scenes of tests/segment_scenes.py at the structural edges of the chunk decomposition (chunk multiples, split nodes, more segments than
chunks), supervoxel nodes, and a scene with dropped clusters (label -1)."""
import ctypes as C
import math

import numpy as np
import pytest

from segment_fields_ref import ref_class_hist, ref_field_stats
from segment_scenes import GROUP, SPLIT, big_nodes, degenerate_scene, fragmented_plane

pytestmark = pytest.mark.gpu

STAT_KEYS = ("n_valid", "anchor", "mean", "var", "vmin", "vmax")
HIST_KEYS = ("hist", "n_outside", "majority", "majority_count")
INT32_MAX = np.iinfo(np.int32).max
U = 2.0 ** -52

SCENES = {
    "big_nodes": lambda gpu: (big_nodes(), 2, GROUP),
    "degenerate": lambda gpu: (degenerate_scene()[0], 2, GROUP),
    "fragmented": lambda gpu: (fragmented_plane(side=48), 2, SPLIT),
    "pc_svgs": lambda gpu: (gpu.scenes.pc_scene(60_000), 3, {}),
    "town": lambda gpu: (gpu.scenes.town_scene(60_000), 2, {}),
}
_cache = {}


def _engine(gpu, xyz, method=2, **kw):
    eng = gpu.Engine(gpu.default_params(method, **kw))
    eng.set_points(xyz)
    eng.run()
    return eng


def _scene(gpu, name):
    """(points, segmented engine, point labels, descriptor table) of a scene, made once and shared; the tests leave it segmented and unchanged."""
    if name not in _cache:
        xyz, method, kw = SCENES[name](gpu)
        eng = _engine(gpu, xyz, method, **kw)
        _cache[name] = (xyz, eng, eng.point_labels(), eng.segment_descriptors())
    return _cache[name]


def _same(a, b):
    return set(a) == set(b) and all(a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def _int_field(n, ch, seed):
    return np.random.default_rng(seed).integers(0, 4096, (n, ch)).astype(np.float32)


def _check_exact(got, field, labels, desc):
    """got against the restatement at got's own anchor, by value: for fields whose d and d * d are integers and whose sums stay below 2^53."""
    K, ch = got["mean"].shape
    assert all(got[k].shape == (K, ch) for k in STAT_KEYS)
    assert [got[k].dtype for k in STAT_KEYS] == [np.int64, np.float64, np.float64, np.float64, np.float32, np.float32]
    finite = field[np.isfinite(field)]
    assert (finite == np.rint(finite)).all() and np.abs(finite).max() <= 4095
    assert int(desc["n_points"].max()) * 4095.0 ** 2 < 2.0 ** 53   # every partial sum of d (|d| <= 4095) and of d * d is an exact integer
    ref = ref_field_stats(field, labels, K, got["anchor"])
    for k in ("n_valid", "mean", "var", "vmin", "vmax"):
        bad = np.nonzero(~((got[k] == ref[k]) | (np.isnan(got[k].astype(np.float64)) & np.isnan(ref[k].astype(np.float64)))))
        assert bad[0].size == 0, (k, bad[0][:5], bad[1][:5], got[k][bad][:5], ref[k][bad][:5])
    return ref


def test_scenes_reach_their_edges(gpu):
    from helpers import SD_CHUNK
    n = _scene(gpu, "big_nodes")[3]["n_points"]
    assert {0, 1, SD_CHUNK - 1} <= set((n % SD_CHUNK).tolist()) and {2047, 2048, 2049, 4096, 4097} <= set(n.tolist()) and (n == 1).any()
    n = _scene(gpu, "degenerate")[3]["n_points"]
    assert n.max() <= 9 and n.min() == 1
    xyz, eng, _, _ = _scene(gpu, "fragmented")
    assert eng.counts()["kept"] >= 48 * 48 and xyz.shape[0] // SD_CHUNK + 1 <= 15   # many more segments than full chunks
    assert _scene(gpu, "pc_svgs")[1].counts()["supervoxels"] > 0
    assert (_scene(gpu, "town")[2] == -1).any()


# ---------------------------------------------------------------- 1. exact against the restatement
@pytest.mark.parametrize("ch", [1, 3, 5, 64])
@pytest.mark.parametrize("name", list(SCENES))
def test_integer_field_equals_the_restatement(gpu, name, ch):
    xyz, eng, labels, desc = _scene(gpu, name)
    field = _int_field(xyz.shape[0], ch, 100 + ch)
    got = eng.segment_field_stats(field if ch > 1 else field[:, 0])
    assert got["mean"].shape == (eng.counts()["kept"], ch)
    ref = _check_exact(got, field, labels, desc)
    assert np.array_equal(ref["n_valid"], np.repeat(desc["n_points"][:, None], ch, axis=1))


@pytest.mark.parametrize("name", list(SCENES))
def test_padded_stride_and_device_tensor(gpu, name):
    torch = pytest.importorskip("torch")
    xyz, eng, labels, desc = _scene(gpu, name)
    ch = 5
    field = _int_field(xyz.shape[0], ch, 7)
    host = eng.segment_field_stats(field)
    _check_exact(host, field, labels, desc)
    wide = np.full((xyz.shape[0], ch + 3), np.float32(np.nan))
    wide[:, :ch] = field
    view = wide[:, :ch]
    assert view.strides == (4 * (ch + 3), 4)
    assert _same(host, eng.segment_field_stats(view))
    dev = torch.from_numpy(field).to("cuda:0")
    assert _same(host, eng.segment_field_stats(dev))
    dwide = torch.from_numpy(wide).to("cuda:0")[:, :ch]
    assert dwide.stride(0) == ch + 3 and _same(host, eng.segment_field_stats(dwide))
    assert _same(eng.segment_field_stats(field[:, 2]), eng.segment_field_stats(dev[:, 2].contiguous()))


# ---------------------------------------------------------------- 2. the anchor
@pytest.mark.parametrize("name", list(SCENES))
def test_anchor_is_one_point_of_the_segment(gpu, name):
    xyz, eng, labels, _ = _scene(gpu, name)
    ch = 5
    field = _int_field(xyz.shape[0], ch, 9)
    rng = np.random.default_rng(10)
    field.reshape(-1)[rng.choice(field.size, field.size // 4, replace=False)] = np.nan   # many anchors meet an invalid value: 0.0 there
    got = eng.segment_field_stats(field)
    K = got["anchor"].shape[0]
    m = labels >= 0
    lab = labels[m].astype(np.int64)
    expect = np.where(np.isfinite(field[m]), field[m].astype(np.float64), 0.0)
    explains = (expect == got["anchor"][lab]).all(axis=1)           # this point explains every channel of its segment's anchor row
    assert (np.bincount(lab[explains], minlength=K) >= 1).all()
    assert (got["anchor"] == 0).any() and (got["anchor"] != 0).any()


# ---------------------------------------------------------------- 3. identities
@pytest.mark.parametrize("name", list(SCENES))
def test_xyz_as_field_gives_the_descriptor_table(gpu, name):
    xyz, eng, labels, d = _scene(gpu, name)
    got = eng.segment_field_stats(xyz)
    assert np.array_equal(got["n_valid"], np.repeat(d["n_points"][:, None], 3, axis=1))
    assert (got["vmin"] == d["bbox6"][:, :3]).all() and (got["vmax"] == d["bbox6"][:, 3:]).all()   # == : a zero of either sign
    # the bars of helpers.check_descriptors for centroid3 and cov6
    assert (np.abs(got["mean"] - d["centroid3"]) <= 1e-9 * (1 + np.linalg.norm(d["centroid3"], axis=1))[:, None]).all()
    tr = d["cov6"][:, [0, 3, 5]].sum(axis=1)
    assert (np.abs(got["var"] - d["cov6"][:, [0, 3, 5]]) <= 1e-8 * tr[:, None] + 1e-30).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_per_segment_constant(gpu, name):
    xyz, eng, labels, d = _scene(gpu, name)
    K = d["n_points"].shape[0]
    v = (np.random.default_rng(12).normal(0.0, 1000.0, K) + 0.1).astype(np.float32)
    field = np.where(labels >= 0, v[np.maximum(labels, 0)], np.float32(np.nan)).astype(np.float32)
    got = eng.segment_field_stats(field)
    assert np.array_equal(got["n_valid"][:, 0], d["n_points"])
    assert (got["var"] == 0).all()
    for k in ("mean", "vmin", "vmax", "anchor"):
        assert np.array_equal(got[k][:, 0].astype(np.float64), v.astype(np.float64)), k


# ---------------------------------------------------------------- 4. general floats
def _exact_square_parts(d):
    """d * d as an unevaluated sum p + e of two doubles (Veltkamp split, Dekker product): exact, so math.fsum over both gives sum d^2 rounded once."""
    c = 134217729.0 * d
    hi = c - (c - d)
    lo = d - hi
    p = d * d
    e = ((hi * hi - p) + 2.0 * hi * lo) + lo * lo
    return p, e


@pytest.mark.parametrize("name", ["big_nodes", "town"])
def test_general_floats_within_the_summation_bound(gpu, name):
    """Channel 0 is the issue's 1e9 + N(0, 1) rounded to float32: floats there are 64 apart, so it is 1e9 throughout, d = 0, and it only
    shows that a large offset costs nothing.  Channels 1 (offset 1e4, floats 1e-3 apart) and 2 (no offset, d of many magnitudes) are the
    ones that exercise the summation: keep them.
    mean and var are tested directly, with the bounds on S1 and S2 carried through the two formulas.  With u = 2^-52 and n terms summed
    in any order: |S1 - S1x| <= e1 = n u sum|d| and |S2 - S2x| <= e2 = n u sum d^2 (the worst case of a summation of n terms with a factor 2
    over the unit roundoff, which also covers the rounding of the products d * d).  m1 = S1 / n is then off by at most e1 / n + u |m1|; the
    mean anchor + m1 by that plus u |mean|; var = S2 / n - m1 m1 by e2 / n + 2 |m1| e1 / n plus one rounding of each of the quotient, the
    product and the difference, each at most u (S2x / n + m1^2).  S1x and S2x are math.fsum over the exact d (a float minus a float of
    the same segment, exact in fp64) and the exact d * d (two doubles per product); the reference's own last steps run in fp64, which
    doubling the rounding terms covers."""
    xyz, eng, labels, d = _scene(gpu, name)
    rng = np.random.default_rng(14)
    N = xyz.shape[0]
    field = np.stack([(1e9 + rng.normal(0, 1, N)).astype(np.float32), (1e4 + rng.normal(0, 1, N)).astype(np.float32),
                      rng.normal(0, 1, N).astype(np.float32)], axis=1)
    got = eng.segment_field_stats(field)
    K = got["mean"].shape[0]
    order = np.argsort(labels, kind="stable")
    start = np.searchsorted(labels[order], np.arange(K + 1))
    worst = 0.0
    for k in range(K):
        idx = order[start[k]:start[k + 1]]
        n = idx.size
        assert n == d["n_points"][k] == got["n_valid"][k, 0]
        for c in range(3):
            a = got["anchor"][k, c]
            dd = field[idx, c].astype(np.float64) - a
            p, e = _exact_square_parts(dd)
            s1x, s2x = math.fsum(dd), math.fsum(np.concatenate([p, e]))
            A1 = math.fsum(np.abs(dd))
            e1, e2 = n * U * A1, n * U * s2x
            m1x = s1x / n
            meanx, varx = a + m1x, max(0.0, s2x / n - m1x * m1x)
            tol_mean = e1 / n + 2 * U * (abs(m1x) + abs(meanx))
            tol_var = e2 / n + 2 * abs(m1x) * e1 / n + 4 * U * (s2x / n + m1x * m1x)
            em, ev = abs(got["mean"][k, c] - meanx), abs(got["var"][k, c] - varx)
            assert em <= tol_mean, (k, c, n, em, tol_mean)
            assert ev <= tol_var, (k, c, n, ev, tol_var)
            if tol_var > 0:
                worst = max(worst, ev / tol_var)
    print(f"{name}: largest var error / bound = {worst:.3g}")
    # the shift does its work: a unit spread on an offset of 1e4 keeps its variance (floats there are 1e-3 apart)
    big = d["n_points"] >= 1000
    assert big.any() and (got["var"][big, 1] > 0.5).all() and (got["var"][big, 1] < 2.0).all()


# ---------------------------------------------------------------- 5. invalid values
@pytest.mark.parametrize("name", ["big_nodes", "fragmented", "town"])
def test_invalid_values_are_skipped(gpu, name):
    xyz, eng, labels, d = _scene(gpu, name)
    N, ch = xyz.shape[0], 3
    clean = _int_field(N, ch, 16)
    rng = np.random.default_rng(17)
    field = clean.copy()
    bad = rng.choice(N * ch, N * ch // 10, replace=False)
    field.reshape(-1)[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), bad.size)
    got = eng.segment_field_stats(field)
    _check_exact(got, field, labels, d)
    K = got["mean"].shape[0]
    m = labels >= 0
    n_bad = np.stack([np.bincount(labels[m], weights=~np.isfinite(field[m, c]), minlength=K) for c in range(ch)], axis=1).astype(np.int64)
    assert n_bad.sum() > 0 and np.array_equal(got["n_valid"], d["n_points"][:, None] - n_bad)
    # one channel of the largest segment invalid throughout: that entry is empty, the segment's other channels and the other segments stay
    k = int(np.argmax(d["n_points"]))
    field2 = field.copy()
    field2[labels == k, 1] = np.nan
    got2 = eng.segment_field_stats(field2)
    assert got2["n_valid"][k, 1] == 0 and got2["anchor"][k, 1] == 0
    assert all(np.isnan(got2[f][k, 1]) for f in ("mean", "var", "vmin", "vmax"))
    keep = np.ones((K, ch), dtype=bool)
    keep[k, 1] = False
    for f in STAT_KEYS:
        assert np.array_equal(got2[f][keep].view(np.uint8), got[f][keep].view(np.uint8)), f
    _check_exact(got2, field2, labels, d)


# ---------------------------------------------------------------- 6. histogram
@pytest.mark.parametrize("n_classes", [1, 7, 1024])
@pytest.mark.parametrize("name", list(SCENES))
def test_class_histogram(gpu, name, n_classes):
    torch = pytest.importorskip("torch")
    xyz, eng, labels, d = _scene(gpu, name)
    N = xyz.shape[0]
    K = d["n_points"].shape[0]
    rng = np.random.default_rng(18 + n_classes)
    cls = rng.integers(-1, n_classes + 1, N).astype(np.int32)       # -1 and n_classes included
    cls[rng.choice(N, max(N // 50, 1), replace=False)] = INT32_MAX
    if name == "town":
        cls[labels == int(np.argmax(d["n_points"]))] = n_classes - 1     # one class for a whole large segment: the ground of a street scene
    by_size = np.argsort(-d["n_points"], kind="stable")
    k_out = int(by_size[1])
    cls[labels == k_out] = -1                                       # every class outside
    k_tie = int(by_size[2])
    tie = np.nonzero(labels == k_tie)[0]
    if n_classes >= 7 and tie.size >= 2:                            # a tie of the two largest counts: the lower class wins
        cls[tie] = np.where(np.arange(tie.size) % 2 == 0, 5, 3)
        if tie.size % 2:
            cls[tie[-1]] = n_classes
    got = eng.segment_class_histogram(cls, n_classes)
    assert [got[k].dtype for k in HIST_KEYS] == [np.int64, np.int64, np.int32, np.int64]
    assert got["hist"].shape == (K, n_classes) and all(got[k].shape == (K,) for k in HIST_KEYS[1:])
    ref = ref_class_hist(cls, labels, K, n_classes)
    for k in HIST_KEYS:
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["hist"].sum(axis=1) + got["n_outside"], d["n_points"])
    assert got["majority"][k_out] == -1 and got["majority_count"][k_out] == 0 and got["n_outside"][k_out] == d["n_points"][k_out]
    if n_classes >= 7 and tie.size >= 2:
        assert got["hist"][k_tie, 3] == got["hist"][k_tie, 5] == tie.size // 2 and got["majority"][k_tie] == 3
    assert got["n_outside"].sum() > 0
    assert _same(got, eng.segment_class_histogram(torch.from_numpy(cls).to("cuda:0"), n_classes))


# ---------------------------------------------------------------- 7. determinism and isolation
def _others(eng):
    off, idx = eng.clusters()
    d, g = eng.segment_descriptors(), eng.segment_graph()
    b = {f: eng.segment_boxes(f) for f in ("principal", "upright")}
    return ([off, idx, eng.point_labels()] + [d[k] for k in sorted(d)] + [g[k] for k in sorted(g)] +
            [b[f][k] for f in sorted(b) for k in sorted(b[f])])


def _eq(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_deterministic_and_without_side_effects(gpu):
    xyz = gpu.scenes.town_scene(60_000)
    N = xyz.shape[0]
    rng = np.random.default_rng(20)
    field = np.stack([(1e9 + rng.normal(0, 1, N)), rng.normal(0, 1, N), rng.uniform(0, 255, N), xyz[:, 2], rng.normal(5, 2, N)], axis=1).astype(np.float32)
    field[rng.choice(N, 100, replace=False), 1] = np.nan
    cls = rng.integers(-1, 17, N).astype(np.int32)
    e1 = _engine(gpu, xyz)
    before = _others(e1)
    s1, h1 = e1.segment_field_stats(field), e1.segment_class_histogram(cls, 16)
    assert _eq(before, _others(e1))                                   # cached tables and labels: byte for byte what they were
    assert _same(s1, e1.segment_field_stats(field)) and _same(h1, e1.segment_class_histogram(cls, 16))   # call to call
    assert _eq(before, _others(e1))
    e2 = _engine(gpu, xyz)                                            # engine to engine; here the new calls come before any other getter
    assert _same(s1, e2.segment_field_stats(field)) and _same(h1, e2.segment_class_histogram(cls, 16))
    assert _eq(before, _others(e2))
    # the next run is unaffected: a second cloud on the first engine, its own stats right
    xyz2 = gpu.scenes.urban_scene(40_000)
    e1.set_points(xyz2)
    with pytest.raises(gpu.VgsError) as e:
        e1.segment_field_stats(field)
    assert e.value.status == gpu._lib.VGS_E_STATE
    e1.run()
    f2 = _int_field(xyz2.shape[0], 3, 21)
    _check_exact(e1.segment_field_stats(f2), f2, e1.point_labels(), e1.segment_descriptors())
    c2 = rng.integers(0, 9, xyz2.shape[0]).astype(np.int32)
    h = e1.segment_class_histogram(c2, 9)
    r = ref_class_hist(c2, e1.point_labels(), e1.counts()["kept"], 9)
    assert all(np.array_equal(h[k], r[k]) for k in HIST_KEYS)


# ---------------------------------------------------------------- 8. state and argument contract
def _raw_stats(eng, field, n, ch, stride, outs=None):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return eng._L.vgs_segment_field_stats(eng._h, p(field), n, ch, stride, *([None] * 6 if outs is None else [p(o) for o in outs]))


def test_state_and_argument_contract(gpu):
    lib = gpu._lib
    xyz = gpu.scenes.town_scene(60_000)
    N = xyz.shape[0]
    field = _int_field(N, 4, 22)
    cls = np.zeros(N, dtype=np.int32)
    eng = gpu.Engine(gpu.default_params(2))
    for call in (lambda: eng.segment_field_stats(field), lambda: eng.segment_class_histogram(cls, 4)):
        with pytest.raises(gpu.VgsError) as e:
            call()
        assert e.value.status == lib.VGS_E_STATE
    eng.set_points(xyz)
    eng.voxelize(); eng.features(); eng.adjacency()
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_field_stats(field)
    assert e.value.status == lib.VGS_E_STATE
    eng.segment()
    bad = [(lambda: eng.segment_field_stats(field[:-1]), "n ="), (lambda: eng.segment_field_stats(np.zeros((N, 0), np.float32)), "n_channels"),
           (lambda: eng.segment_field_stats(np.zeros((N, 65), np.float32)), "n_channels"),
           (lambda: eng.segment_class_histogram(cls[:-1], 4), "n ="), (lambda: eng.segment_class_histogram(cls, 0), "n_classes"),
           (lambda: eng.segment_class_histogram(cls, 1025), "n_classes")]
    for call, word in bad:
        with pytest.raises(gpu.VgsError) as e:
            call()
        assert e.value.status == lib.VGS_E_ARG and word in str(e.value), (word, str(e.value))
    for stride in (12, 4 * 4 + 2, 0, -16):          # below 4 * C; not a multiple of 4
        assert _raw_stats(eng, field, N, 4, stride) == lib.VGS_E_ARG, stride
        assert b"stride_bytes" in eng._L.vgs_last_error_string(eng._h)
    assert _raw_stats(eng, field, N, 4, 16) == lib.VGS_OK             # every output NULL
    assert eng.segment_field_stats(np.zeros((N, 64), np.float32))["mean"].shape[1] == 64
    assert eng.segment_class_histogram(cls, 1024)["hist"].shape[1] == 1024
    # the device entry points check the same arguments
    torch = pytest.importorskip("torch")
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_field_stats(torch.zeros((N - 1, 2), dtype=torch.float32, device="cuda:0"))
    assert e.value.status == lib.VGS_E_ARG
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_class_histogram(torch.zeros(N, dtype=torch.int32, device="cuda:0"), 1025)
    assert e.value.status == lib.VGS_E_ARG
    # no kept segment: OK, nothing written
    e0 = _engine(gpu, xyz, voxels_min=10_000_000)
    assert e0.counts()["kept"] == 0
    outs = [np.full(8, 7, dtype=dt) for dt in (np.int64, np.float64, np.float64, np.float64, np.float32, np.float32)]
    assert _raw_stats(e0, field, N, 4, 16, outs) == lib.VGS_OK and all((o == 7).all() for o in outs)
    houts = [np.full(8, 7, dtype=dt) for dt in (np.int64, np.int64, np.int32, np.int64)]
    assert e0._L.vgs_segment_class_histogram(e0._h, cls.ctypes.data_as(C.c_void_p), N, 4, *(o.ctypes.data_as(C.c_void_p) for o in houts)) == lib.VGS_OK
    assert all((o == 7).all() for o in houts)
    s0, h0 = e0.segment_field_stats(field), e0.segment_class_histogram(cls, 4)
    assert all(s0[k].shape == (0, 4) for k in STAT_KEYS) and h0["hist"].shape == (0, 4) and h0["majority"].shape == (0,)


def test_too_many_counters_are_unsupported(gpu):
    """K * n_classes above 2^27: 363 x 363 one-voxel segments (and the first point's own) are more than 2^27 / 1024 = 131 072."""
    xyz = fragmented_plane(side=363)
    eng = _engine(gpu, xyz, **SPLIT)
    K = eng.counts()["kept"]
    assert K > (1 << 27) // 1024
    cls = np.zeros(xyz.shape[0], dtype=np.int32)
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_class_histogram(cls, 1024)
    assert e.value.status == gpu._lib.VGS_E_UNSUPPORTED and str(K) in str(e.value) and str(K * 1024) in str(e.value)
    nc = (1 << 27) // K + 1                             # the first class count that no longer fits
    with pytest.raises(gpu.VgsError) as e:
        eng.segment_class_histogram(cls, nc)
    assert e.value.status == gpu._lib.VGS_E_UNSUPPORTED
    h = eng.segment_class_histogram(cls, 4)             # the same call with a table that fits
    assert np.array_equal(h["hist"][:, 0], eng.segment_descriptors()["n_points"]) and h["hist"][:, 1:].sum() == 0


def test_tile_context_is_refused(gpu):
    xyz = gpu.scenes.town_scene(60_000)
    eng = gpu.Engine(gpu.default_params(2))
    eng.set_points(xyz)
    lo = np.array([-1e9, -1e9], dtype=np.float64)
    hi = np.array([1e9, 1e9], dtype=np.float64)
    eng._ck(eng._L.vgs_set_owned_region(eng._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    eng.run()
    for call in (lambda: eng.segment_field_stats(xyz), lambda: eng.segment_class_histogram(np.zeros(xyz.shape[0], np.int32), 3)):
        with pytest.raises(gpu.VgsError) as e:
            call()
        assert e.value.status == gpu._lib.VGS_E_STATE and "tile context" in str(e.value)
