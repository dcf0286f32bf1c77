"""Per-segment descriptors across the ranks of the native tiled driver (vgs_tiles_get_segment_descriptors, include/vgs_tiles.h), ranks as
threads of this process over LocalGroup on one GPU:
  * 2x1, 2x2 and 4x2 layouts of scenes.tiled_urban_scene: every rank's table has the same bytes; counts, exact boxes, centroid, covariance,
    eigenpairs and features match numpy float64 on the gathered points; n_nodes counts the shared grid's voxels of each segment; the
    table survives a second call and a second run bit for bit, and neither the size query nor a cached call waits for a peer;
  * the same layout 3e5 / 5e5 m from the origin;
  * one rank: equal to a plain engine's vgs_get_segment_descriptors;
  * an injected failure in the descriptor phase takes the peer out with it;
  * examples/vgs_tiles_run --segments writes rank 0's table."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from helpers import ref_descriptors, ref_features

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")
N_PER = 60_000


def _pitch(n_per):
    return 50.0 * np.sqrt(n_per / 10_000_000)


def _parts(gpu, tiles, n_per=N_PER, shift=None):
    world = tiles[0] * tiles[1]
    parts = [gpu.scenes.tiled_urban_scene(n_per * world, tiles=tiles, tile_index=r) for r in range(world)]
    if shift is not None:
        parts = [(p.astype(np.float64) + np.asarray(shift)).astype(np.float32) for p in parts]
    return parts


def _ranks(gpu, tiles, pitch, parts, body, center=(0.0, 0.0), timeout=300.0, params=None):
    """one rank of the native driver per tile, threads of this process; body(rank, driver, points) -> anything.  Exceptions come back as
    results; a rank still inside the driver after `timeout` fails the test."""
    from vgs_svgs_segmentation_amd import tiles_native as tn
    world = tiles[0] * tiles[1]
    grp = tn.LocalGroup(world)
    out = [None] * world

    def rank_main(r):
        try:
            p = params if params is not None else gpu.default_params(2, voxel_size=0.1)
            t = tn.NativeTiles(p, tn.COMM_LOCAL, grp.handle, r, world, tiles, pitch, center=center)
            try:
                out[r] = body(r, t, parts[r])
            finally:
                t.close()
        except Exception as ex:  # noqa: BLE001
            out[r] = ex
    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout)
    hung = [r for r, t in enumerate(th) if t.is_alive()]
    if hung:
        grp.abort()
        pytest.fail(f"rank(s) {hung} still inside the driver after {timeout} s")
    grp.close()
    return out


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def _size_query(t):
    K = C.c_int64(-1)
    assert t._L.vgs_tiles_get_segment_descriptors(t._h, C.byref(K), *([None] * 8)) == 0
    return K.value


def _collect(r, t, xyz):
    t.set_points(xyz)
    t.run()
    labels, kept = t.point_labels()
    first = t.segment_descriptors()
    if r == 0:
        # neither the size query nor a cached call is a collective: rank 0 alone must come back
        assert _size_query(t) == kept
        assert _same(t.segment_descriptors(), first)
    second = t.segment_descriptors()
    labels_after, _ = t.point_labels()
    t.run()
    labels2, kept2 = t.point_labels()
    third = t.segment_descriptors()
    return dict(labels=labels, kept=kept, d=first, second=_same(first, second), rerun=_same(first, third),
                labels_equal=bool(np.array_equal(labels, labels_after) and np.array_equal(labels, labels2) and kept2 == kept),
                times=t.descriptor_times())


def _check_against_points(gpu, parts, out, params=None):
    world = len(parts)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    kept = out[0]["kept"]
    d = out[0]["d"]
    for o in out:
        assert o["kept"] == kept and _same(o["d"], d)      # every rank: the same bytes
        assert o["second"] and o["rerun"] and o["labels_equal"]
    labels = np.concatenate([o["labels"] for o in out])
    xyz = np.concatenate(parts)
    assert kept > 0 and labels.max() == kept - 1
    ref = ref_descriptors(xyz, labels, kept)
    assert np.array_equal(d["n_points"], np.bincount(labels[labels >= 0], minlength=kept))
    assert np.array_equal(d["bbox6"].view(np.uint32), ref["bbox6"].view(np.uint32))
    c = d["centroid3"]
    assert (np.abs(c - ref["centroid3"]) <= 1e-9 * (1 + np.linalg.norm(ref["centroid3"], axis=1))[:, None]).all()
    tr = ref["cov6"][:, [0, 3, 5]].sum(axis=1)
    assert (np.abs(d["cov6"] - ref["cov6"]) <= 1e-8 * tr[:, None] + 1e-30).all()
    lmax = ref["evals3"][:, 2]
    assert (d["evals3"] >= 0).all() and (np.diff(d["evals3"], axis=1) >= 0).all()
    assert (np.abs(d["evals3"] - np.maximum(ref["evals3"], 0)) <= 1e-8 * lmax[:, None] + 1e-30).all()
    V = d["evecs9"].reshape(kept, 3, 3)
    assert np.allclose(np.einsum("kri,krj->kij", V, V), np.eye(3)[None], atol=1e-10)
    for j in range(3):
        col = V[:, :, j]
        assert (col[np.arange(kept), np.argmax(np.abs(col), axis=1)] > 0).all(), j
        w = ref["evals3"]
        gap = np.minimum(np.abs(w[:, j] - w[:, j - 1]) if j > 0 else np.inf, np.abs(w[:, j + 1] - w[:, j]) if j < 2 else np.inf)
        sel = gap >= 1e-3 * lmax
        assert (np.abs((col * ref["evecs"][:, :, j]).sum(axis=1))[sel] >= 1 - 1e-6).all(), j
    one = d["n_points"] == 1
    assert (d["cov6"][one] == 0).all() and (V[one] == np.eye(3)[None]).all()
    np.testing.assert_allclose(d["eigen8"], ref_features(d["evals3"], False), rtol=1e-5, atol=1e-6)
    # n_nodes: the distinct voxels of the shared grid among each segment's points -- the grid of one engine over the union, rank order
    eng = gpu.Engine(params if params is not None else gpu.default_params(2, voxel_size=0.1))
    eng.set_points(xyz)
    eng.run()
    pv = eng.point_voxel()
    m = (labels >= 0) & (pv >= 0)
    pairs = np.unique(labels[m].astype(np.int64) * (int(pv.max()) + 1) + pv[m])
    assert np.array_equal(d["n_nodes"], np.bincount(pairs // (int(pv.max()) + 1), minlength=kept).astype(np.int32))
    # at least one checked segment spans two ranks
    rank_of = np.repeat(np.arange(world), [p.shape[0] for p in parts])
    lab_ranks = np.zeros((kept, world), bool)
    lab_ranks[labels[labels >= 0], rank_of[labels >= 0]] = True
    assert (lab_ranks.sum(axis=1) >= 2).any()
    return d


@pytest.mark.parametrize("tiles", [(2, 1), (2, 2), (4, 2)], ids=["2x1", "2x2", "4x2"])
def test_tiled_descriptors_match_the_gathered_points(gpu, tiles):
    parts = _parts(gpu, tiles)
    out = _ranks(gpu, tiles, _pitch(N_PER), parts, _collect)
    _check_against_points(gpu, parts, out)
    for o in out:
        assert o["times"]["total"] > 0 and o["times"]["exchange"] >= 0


def test_tiled_descriptors_far_from_the_origin(gpu):
    shift = (3e5, 5e5, 50.0)
    parts = _parts(gpu, (2, 2), shift=shift)
    out = _ranks(gpu, (2, 2), _pitch(N_PER), parts, _collect, center=shift[:2])
    _check_against_points(gpu, parts, out)


def test_one_rank_equals_a_plain_engine(gpu):
    xyz = gpu.scenes.urban_scene(200_000)
    out = _ranks(gpu, (1, 1), 1000.0, [xyz], lambda r, t, p: (t.set_points(p), t.run(), t.point_labels(), t.segment_descriptors())[2:])
    assert not isinstance(out[0], Exception), out[0]
    (labels, kept), d = out[0]
    eng = gpu.Engine(gpu.default_params(2, voxel_size=0.1))
    eng.set_points(xyz)
    eng.run()
    assert np.array_equal(labels, eng.point_labels()) and kept == eng.counts()["kept"]
    ref = eng.segment_descriptors()
    assert set(d) == set(ref)
    for name in ref:
        assert np.array_equal(d[name], ref[name]), name


def test_a_failing_rank_in_the_descriptor_phase_takes_its_peer_out(gpu, monkeypatch):
    monkeypatch.setenv("VGS_TILES_FAIL_RANK", "1")
    monkeypatch.setenv("VGS_TILES_FAIL_AT", "descriptors")
    parts = _parts(gpu, (2, 1))

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        t.segment_descriptors()
        return "finished"
    out = _ranks(gpu, (2, 1), _pitch(N_PER), parts, body, timeout=120.0)
    assert isinstance(out[1], gpu.VgsError) and "VGS_E_STATE" in str(out[1]) and "descriptors" in str(out[1]), out[1]
    assert isinstance(out[0], gpu.VgsError) and "VGS_E_PEER" in str(out[0]) and "rank 1" in str(out[0]), out[0]


def test_descriptors_before_a_run_are_refused_without_a_collective(gpu):
    from vgs_svgs_segmentation_amd import tiles_native as tn
    grp = tn.LocalGroup(2)
    t = tn.NativeTiles(gpu.default_params(2, voxel_size=0.1), tn.COMM_LOCAL, grp.handle, 0, 2, (2, 1), 5.0)
    try:
        assert _size_query(t) == 0
        with pytest.raises(gpu.VgsError, match="VGS_E_STATE"):
            t._ck(t._L.vgs_tiles_get_segment_descriptors(t._h, None, np.zeros(1, np.int64).ctypes.data_as(C.c_void_p), *([None] * 7)))
    finally:
        t.close()
        grp.close()


def test_tiles_run_front_end_writes_the_table(gpu, tmp_path):
    tiles = (2, 2)
    parts = _parts(gpu, tiles)
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    prefix = str(tmp_path / "t")
    for r, p in enumerate(parts):
        np.ascontiguousarray(p, dtype=np.float32).tofile(f"{prefix}.{r}.f32")
    csv = str(tmp_path / "seg.csv")
    out = subprocess.check_output([EXE, "--emulate", "2x2", "--pitch", repr(float(_pitch(N_PER))), "--voxel", "0.1", "--segments", csv, prefix],
                                  text=True, timeout=300)
    kept = int(out.strip().splitlines()[-1].split()[1])
    d = _ranks(gpu, tiles, _pitch(N_PER), parts, lambda r, t, p: (t.set_points(p), t.run(), t.segment_descriptors())[2])[0]
    assert not isinstance(d, Exception), d
    tab = np.loadtxt(csv, delimiter=",", skiprows=1, ndmin=2)
    assert tab.shape == (kept, 29) and kept == d["n_points"].size
    assert np.array_equal(tab[:, 0], np.arange(kept))
    assert np.array_equal(tab[:, 1].astype(np.int64), d["n_points"]) and np.array_equal(tab[:, 2].astype(np.int32), d["n_nodes"])
    assert np.array_equal(tab[:, 3:9].astype(np.float32), d["bbox6"])
    assert np.array_equal(tab[:, 9:12], d["centroid3"]) and np.array_equal(tab[:, 12:15], d["evals3"])
    V = d["evecs9"].reshape(kept, 3, 3)
    assert np.array_equal(tab[:, 15:18], V[:, :, 0]) and np.array_equal(tab[:, 18:21], V[:, :, 2])
    assert np.array_equal(tab[:, 21:29].astype(np.float32), d["eigen8"])
