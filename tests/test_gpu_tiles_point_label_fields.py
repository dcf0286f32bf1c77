"""Field statistics and class histograms of any per-point labelling across the ranks of the native tiled driver
(vgs_tiles_point_label_field_stats, vgs_tiles_point_label_class_histogram; include/vgs_tiles.h), ranks as threads of this process over
LocalGroup on one GPU.  Every rank hands in the labels and the attribute rows of its own points only; only per-label records cross.  The
reference is tests/segment_fields_ref.py over the gathered octree points (the finite ones), evaluated at the table's own anchor.
  1. 2x1, 2x2 and 2x2 far from the origin: two labels inside every voxel, integer fields of 1, 5 and 64 channels and histograms of 1, 16 and
     1024 classes by ==; every rank the same bytes; a second call and a second run; side effects; own records, their fold and finish;
  2. one rank: a plain engine's tables byte for byte; the driver's own labels give the node tables;
  3. the driver's refined labels on 2x2;
  4. designed scenes at the chunk and fold limits, with voxels that two and four ranks share, invalid values, stride and device tensors;
  5. general floats against math.fsum within the summation bound test_gpu_tiles_segfields.py carries through the fold;
  6. the status contract;  7. the front end."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from segment_fields_ref import ref_class_hist, ref_field_stats
from segment_scenes import BIG_NODES, FAR, GROUP
from test_gpu_point_label_fields import HIST_KEYS, STAT_KEYS, U, _exact_square_parts, _int_field
from test_gpu_segment_limits import _split
from test_gpu_tiles_point_label_tables import CENTER, FILL, SIZES, _designed_scene, _mixed_labels, _offsets, _ref_ids
from test_gpu_tiles_segdesc import _parts, _pitch, _ranks, _same
from test_gpu_tiles_segfields import _finish

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")
N_PER = 60_000
SD_CHUNK = 2048
CHANNELS = (1, 5, 64)
CLASSES = (1, 16, 1024)
FRAMES = ("principal", "upright")


def _fields(parts, channels=CHANNELS):
    return {ch: [_int_field(p.shape[0], ch, 2000 * ch + r) for r, p in enumerate(parts)] for ch in channels}


def _classes(parts, classes=CLASSES):
    """per class count, per rank: classes drawn from -2 .. n_classes + 1"""
    return {nc: [np.random.default_rng(9000 + 10 * nc + r).integers(-2, nc + 2, p.shape[0]).astype(np.int32) for r, p in enumerate(parts)]
            for nc in classes}


def _sk(d):
    """a table without its n_skipped (an int): what _same compares"""
    return {k: v for k, v in d.items() if k != "n_skipped"}


def _same_t(a, b):
    return _same(_sk(a), _sk(b)) and a["n_skipped"] == b["n_skipped"]


def _own_first(parts, r, tiles, pitch, center, halo):
    """the number of lower ranks' points inside rank r's region widened by the halo: the driver's own_first of that rank (the local cloud
    is the lower ranks' strips, the own points, the higher ranks' strips)"""
    i, j = r % tiles[0], r // tiles[0]
    big = 1e300
    x0, y0 = center[0] + (i - tiles[0] / 2) * pitch, center[1] + (j - tiles[1] / 2) * pitch
    lo = (x0 if i > 0 else -big, y0 if j > 0 else -big)
    hi = (x0 + pitch if i < tiles[0] - 1 else big, y0 + pitch if j < tiles[1] - 1 else big)
    n = 0
    for p in parts[:r]:
        x, y = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
        n += int(((x >= lo[0] - halo) & (x < hi[0] + halo) & (y >= lo[1] - halo) & (y < hi[1] + halo)).sum())
    return n


def _check_fields(got, field, lab_in, K, n_points):
    """a tiled field table against the restatement over the gathered octree points at the table's own anchor, by ==: integer fields"""
    ch = field.shape[1]
    assert all(got[k].shape == (K, ch) for k in STAT_KEYS)
    assert [got[k].dtype for k in STAT_KEYS] == [np.int64, np.float64, np.float64, np.float64, np.float32, np.float32]
    finite = field[np.isfinite(field)]
    assert (finite == np.rint(finite)).all() and np.abs(finite).max() <= 4095
    assert int(n_points.max(initial=0)) * 4095.0 ** 2 < 2.0 ** 53   # every partial sum and every shift term of the fold: an exact integer
    ref = ref_field_stats(field, lab_in, K, got["anchor"])
    for k in ("n_valid", "mean", "var", "vmin", "vmax"):
        g, w = got[k].astype(np.float64), ref[k].astype(np.float64)
        bad = np.nonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))
        assert bad[0].size == 0, (k, bad[0][:5], bad[1][:5], got[k][bad][:5], ref[k][bad][:5])
    assert (got["n_valid"] <= n_points[:, None]).all()
    empty = n_points == 0
    assert (got["n_valid"][empty] == 0).all() and (got["anchor"][empty] == 0).all()
    assert all(np.isnan(got[k][empty]).all() for k in ("mean", "var", "vmin", "vmax"))


def _check_hist(got, cls, lab_in, K, nc, n_points):
    assert [got[k].dtype for k in HIST_KEYS] == [np.int64, np.int64, np.int32, np.int64]
    ref = ref_class_hist(cls, lab_in, K, nc)
    for k in HIST_KEYS:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (nc, k)
    assert np.array_equal(got["hist"].sum(axis=1) + got["n_outside"], n_points)


def _check_own_and_fold(gpu, out, lab_parts, fin_parts, K, F, CL, stats, hist):
    """each rank's own records name exactly the labels of its own octree points; folded, then finished, they are the table"""
    from vgs_svgs_segmentation_amd import tiles_native as tn
    for r, o in enumerate(out):
        want = np.unique(lab_parts[r][(lab_parts[r] >= 0) & fin_parts[r]])
        for ch in F:
            assert np.array_equal(o["own"][ch]["label"], want), (ch, r)
            assert o["own"][ch]["n_skipped"] == int(((lab_parts[r] >= 0) & ~fin_parts[r]).sum())
        for nc in CL:
            assert np.array_equal(o["own_h"][nc]["label"], want), (nc, r)
    for ch in F:
        folded = tn.fold_field_moments([_sk(o["own"][ch]) for o in out], K, ch)
        assert np.array_equal(folded["n_valid"], stats[ch]["n_valid"])
        assert np.array_equal(folded["anchor"].view(np.uint64), stats[ch]["anchor"].view(np.uint64))
        fin = _finish(gpu, folded, K, ch)
        for k in ("mean", "var", "vmin", "vmax"):
            assert np.array_equal(fin[k].view(np.uint8), stats[ch][k].view(np.uint8)), (ch, k)
    for nc in CL:
        folded = tn.fold_class_counts([_sk(o["own_h"][nc]) for o in out], K, nc)
        for k in HIST_KEYS:
            assert np.array_equal(folded[k], hist[nc][k]), (nc, k)


# ---------------------------------------------------------------- 1. layouts
@pytest.mark.parametrize("layout", ["2x1", "2x2", "2x2_far"])
def test_layouts_equal_the_restatement_over_the_gathered_points(gpu, layout):
    tiles = (2, 1) if layout == "2x1" else (2, 2)
    shift = FAR if layout.endswith("far") else None
    parts = _parts(gpu, tiles, n_per=N_PER, shift=shift)
    bad = np.array([[np.nan, 1.0, 1.0]], np.float32)
    parts = [np.concatenate([p, bad]) for p in parts]   # one point per rank outside the octree, labelled below
    off = _offsets(parts)
    F, CL = _fields(parts), _classes(parts)

    def tables(t, r, lab, K):
        return ({ch: t.label_field_stats(lab, F[ch][r] if ch > 1 else F[ch][r][:, 0], K) for ch in F},
                {nc: t.label_class_histogram(lab, CL[nc][r], nc, K) for nc in CL})

    def same(a, b):
        return all(_same_t(a[0][ch], b[0][ch]) for ch in F) and all(_same_t(a[1][nc], b[1][nc]) for nc in CL)

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        pl, kept = t.point_labels()
        K = 2 * kept + 3
        lab, ref = _mixed_labels(pl, off[r], 1), _ref_ids(off[r], xyz.shape[0])
        d, g = t.segment_descriptors(), t.segment_graph()
        b = {f: t.segment_boxes(f) for f in FRAMES}
        t.refine_labels()
        refined = t.refined_labels().copy()
        cmp_ = t.compare_labels(ref)
        n_points = t.describe_labels(lab, K)["n_points"]
        first = tables(t, r, lab, K)
        times, pay = t.field_times(), t.field_payload()
        second = same(tables(t, r, lab, K), first)
        own = {ch: t.own_point_label_field_moments(K, lab, F[ch][r]) for ch in F}
        own_h = {nc: t.own_point_label_class_counts(K, lab, CL[nc][r], nc) for nc in CL}
        pl2, _ = t.point_labels()
        last = t.label_comparison(cmp_["cell_seg"].size, cmp_["ref_id"].size, kept)
        untouched = (np.array_equal(pl, pl2) and np.array_equal(refined, t.refined_labels()) and _same(d, t.segment_descriptors()) and
                     _same(g, t.segment_graph()) and all(_same(b[f], t.segment_boxes(f)) for f in FRAMES) and
                     _same(last, {k: v for k, v in cmp_.items() if k != "summary"}))
        t.run()
        rerun = same(tables(t, r, lab, K), first)
        return dict(kept=kept, K=K, lab=lab, n_points=n_points, t=first, second=second, rerun=rerun, untouched=untouched, own=own, own_h=own_h,
                    times=times, pay=pay)
    center = shift[:2] if shift else (0.0, 0.0)
    out = _ranks(gpu, tiles, _pitch(N_PER), parts, body, center=center)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    K, world = out[0]["K"], len(parts)
    stats, hist = out[0]["t"]
    for r, o in enumerate(out):
        assert o["K"] == K and same(o["t"], out[0]["t"]), r          # every rank: the same bytes
        assert o["second"] and o["rerun"] and o["untouched"], r
        assert o["times"]["total"] > 0
        # the wire size of the call the getter last saw (the histogram of the last class count): a 40-byte header, 16 + 8 n_classes bytes a record
        assert o["pay"]["bytes_sent"] == 40 + o["pay"]["own_records"] * (16 + 8 * list(CL)[-1]), (r, o["pay"])
    xyz = np.concatenate(parts)
    lab = np.concatenate([o["lab"] for o in out])
    fin = np.isfinite(xyz).all(axis=1)
    lab_in = np.where(fin, lab, -1).astype(np.int32)
    n_points = out[0]["n_points"]
    assert np.array_equal(n_points, np.bincount(lab_in[lab_in >= 0], minlength=K))
    for ch in F:
        got = stats[ch]
        assert got["n_skipped"] == world
        _check_fields(_sk(got), np.concatenate(F[ch]), lab_in, K, n_points)
        assert (got["n_valid"][-3:] == 0).all() and (got["anchor"][-3:] == 0).all()    # three labels no point carries anywhere
        assert all(np.isnan(got[k][-3:]).all() for k in ("mean", "var", "vmin", "vmax"))
    for nc in CL:
        assert hist[nc]["n_skipped"] == world
        _check_hist(_sk(hist[nc]), np.concatenate(CL[nc]), lab_in, K, nc, n_points)
        assert hist[nc]["n_outside"].sum() > 0
    lab_parts = [o["lab"] for o in out]
    fin_parts = [np.isfinite(p).all(axis=1) for p in parts]
    _check_own_and_fold(gpu, out, lab_parts, fin_parts, K, F, CL, {ch: _sk(stats[ch]) for ch in F}, {nc: _sk(hist[nc]) for nc in CL})
    rank_of = np.repeat(np.arange(world), [p.shape[0] for p in parts])
    on = np.zeros((K, world), bool)
    on[lab_in[lab_in >= 0], rank_of[lab_in >= 0]] = True
    assert (on.sum(axis=1) >= 2).any()                      # a checked label has points on two ranks
    prm = gpu.default_params(2, voxel_size=0.1)
    assert any(_own_first(parts, r, tiles, _pitch(N_PER), center, 2 * float(prm.graph_size) + float(prm.voxel_size)) > 0 for r in range(1, world))


# ---------------------------------------------------------------- 2. one rank
def test_one_rank_equals_a_plain_engine(gpu):
    torch = pytest.importorskip("torch")
    xyz = gpu.scenes.urban_scene(120_000)
    N = xyz.shape[0]
    field = _int_field(N, 5, 61)
    rng = np.random.default_rng(62)
    field.reshape(-1)[rng.choice(field.size, field.size // 10, replace=False)] = np.nan
    general = np.stack([(1e4 + rng.normal(0, 1, N)), rng.normal(0, 1, N)], axis=1).astype(np.float32)
    cls = rng.integers(-2, 18, N).astype(np.int32)

    def body(r, t, p):
        t.set_points(p)
        t.run()
        pl, kept = t.point_labels()
        K = 2 * kept + 3
        lab = _mixed_labels(pl, 0, 0)
        o = dict(pl=pl, kept=kept, K=K, lab=lab, s=t.label_field_stats(lab, field, K), g=t.label_field_stats(lab, general, K),
                 h=t.label_class_histogram(lab, cls, 16, K))
        dl = torch.from_numpy(lab).to("cuda:0")
        o["dev"] = (_same_t(t.label_field_stats(dl, torch.from_numpy(field).to("cuda:0"), K), o["s"]) and
                    _same_t(t.label_class_histogram(dl, torch.from_numpy(cls).to("cuda:0"), 16, K), o["h"]))
        o["own"] = (t.label_field_stats(pl, general, kept), t.label_class_histogram(pl, cls, 16, kept))
        o["node"] = (t.segment_field_stats(general), t.segment_class_histogram(cls, 16))
        return o
    o = _ranks(gpu, (1, 1), 1000.0, [xyz], body)[0]
    assert not isinstance(o, Exception), o
    assert o["dev"]
    eng = gpu.Engine(gpu.default_params(2, voxel_size=0.1))
    eng.set_points(xyz)
    eng.run()
    assert np.array_equal(o["pl"], eng.point_labels()) and o["kept"] == eng.counts()["kept"] > 0
    K, lab = o["K"], o["lab"]
    assert _same_t(o["s"], eng.label_field_stats(lab, field, K=K))         # the anchor included
    assert _same_t(o["g"], eng.label_field_stats(lab, general, K=K))
    assert _same_t(o["h"], eng.label_class_histogram(lab, cls, 16, K=K))
    # handed the driver's own point labels with K = kept: the node tables of the tiled driver
    assert o["own"][0]["n_skipped"] == 0 and _same(_sk(o["own"][0]), o["node"][0])
    assert o["own"][1]["n_skipped"] == 0 and _same(_sk(o["own"][1]), o["node"][1])


# ---------------------------------------------------------------- 3. the refined labels
def test_the_drivers_refined_labels(gpu):
    tiles = (2, 2)
    parts = _parts(gpu, tiles, n_per=N_PER)
    F, CL = _fields(parts, (5,)), _classes(parts, (16,))

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        pl, kept = t.point_labels()
        counts = t.refine_labels()
        fine = t.refined_labels().copy()
        return dict(kept=kept, pl=pl, fine=fine, counts=counts, n_points=t.describe_labels(fine, kept)["n_points"],
                    s=t.label_field_stats(fine, F[5][r], kept), h=t.label_class_histogram(fine, CL[16][r], 16, kept))
    out = _ranks(gpu, tiles, _pitch(N_PER), parts, body)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
        assert _same_t(o["s"], out[0]["s"]) and _same_t(o["h"], out[0]["h"])
    kept = out[0]["kept"]
    fine, pl = np.concatenate([o["fine"] for o in out]), np.concatenate([o["pl"] for o in out])
    assert sum(o["counts"]["points_filled"] + o["counts"]["points_changed"] for o in out) > 0 and not np.array_equal(fine, pl)
    n_points = out[0]["n_points"]
    assert np.array_equal(n_points, np.bincount(fine[fine >= 0], minlength=kept))
    assert out[0]["s"]["n_skipped"] == 0
    _check_fields(_sk(out[0]["s"]), np.concatenate(F[5]), fine, kept, n_points)
    _check_hist(_sk(out[0]["h"]), np.concatenate(CL[16]), fine, kept, 16, n_points)


# ---------------------------------------------------------------- 4. structural limits on designed scenes
K_DESIGNED = 40


def _designed_labels(parts):
    """per rank the labels of its own points (the cases of test_gpu_tiles_point_label_tables._designed_labels that bear on attributes):
    0: both sides of a voxel two ranks share; 1 / 2: one side each; 3 / 4: one side alternates inside the shared voxel; 5: one side only,
    the other all negative; 6 / 7: the voxel four ranks share, 6 on ranks 0, 1 and 2, alternating with 7 on rank 2, rank 3 negative;
    8: one point on each of ranks 0 and 1; 10 + 5 r + s: SIZES[s] points on rank r alone; 9 and 30 ..: no point"""
    labs = []
    for r, p in enumerate(parts):
        n = p.shape[0]
        j = np.arange(n)
        lab = np.full(n, -1, np.int64)
        left = r % 2 == 0
        vox0 = np.abs(p[:, 0] - 0.05) < 0.01
        grp = lambda g: vox0 & (np.abs(p[:, 1] - ((g + 1) * 3.0 + 0.05)) < 0.01)   # noqa: E731
        lab[grp(5)] = 0
        lab[grp(4)] = 1 if left else 2
        lab[grp(3)] = np.where(j % 2 == 0, 3, 4)[grp(3)] if left else 3
        lab[grp(8)] = -1 if left else 5
        corner = vox0 & (np.abs(p[:, 1] - CENTER[1]) < 0.01)
        assert corner.sum() > 500
        lab[corner] = (6, 6, -1, -3)[r]
        if r == 2:
            lab[corner] = np.where(j % 2 == 0, 6, 7)[corner]
        fill = np.flatnonzero((np.abs(p[:, 0] - FILL[r][0]) < 0.6) & (np.abs(p[:, 1] - FILL[r][1]) < 0.6))
        at = 0
        for s, size in enumerate(SIZES):
            lab[fill[at:at + size]] = 10 + 5 * r + s
            at += size
        if r < 2:
            lab[fill[at]] = 8
        labs.append(np.ascontiguousarray(lab.astype(np.int32)))
    return labs


def test_structural_limits_and_shared_voxels_on_designed_scenes(gpu):
    torch = pytest.importorskip("torch")
    assert {SD_CHUNK - 1, SD_CHUNK, SD_CHUNK + 1, 64 * SD_CHUNK + 1} <= set(SIZES)
    params = gpu.default_params(2, **GROUP)
    xyz = _designed_scene()
    parts = _split(xyz, CENTER)
    labs = _designed_labels(parts)
    F, CL = _fields(parts, (5,)), _classes(parts, (16,))
    # invalid values.  Label 0 lies on ranks 0 and 1: rank 0's whole share is NaN or +-inf in channel 1, so the anchor there is rank 1's.
    # Label 6 (ranks 0, 1 and 2) is invalid everywhere in channel 2.
    for r in range(4):
        f = F[5][r]
        if r == 0:
            idx = np.flatnonzero(labs[r] == 0)
            f[idx, 1] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(idx.size) % 3]
        f[labs[r] == 6, 2] = np.nan
    assert (labs[0] == 0).any() and (labs[1] == 0).any() and np.isfinite(F[5][1][labs[1] == 0, 1]).all()

    def body(r, t, p):
        t.set_points(p)
        t.run()
        lab, f, c = labs[r], F[5][r], CL[16][r]
        K = K_DESIGNED
        o = dict(s=t.label_field_stats(lab, f, K), h=t.label_class_histogram(lab, c, 16, K), n_points=t.describe_labels(lab, K)["n_points"],
                 own={5: t.own_point_label_field_moments(K, lab, f)}, own_h={16: t.own_point_label_class_counts(K, lab, c, 16)},
                 n_local=t.counts()["points"])
        o["pay"] = t.field_payload()
        wide = np.full((p.shape[0], 8), np.float32(np.nan))
        wide[:, :5] = f
        assert wide[:, :5].strides == (32, 4)
        o["wide"] = _same_t(t.label_field_stats(lab, wide[:, :5], K), o["s"])
        dl = torch.from_numpy(lab).to("cuda:0")
        dwide = torch.from_numpy(wide).to("cuda:0")[:, :5]
        assert dwide.stride(0) == 8
        o["dev"] = (_same_t(t.label_field_stats(dl, torch.from_numpy(f).to("cuda:0"), K), o["s"]) and _same_t(t.label_field_stats(dl, dwide, K), o["s"]) and
                    _same_t(t.label_class_histogram(dl, torch.from_numpy(c).to("cuda:0"), 16, K), o["h"]))
        o["k1"] = t.label_field_stats(np.where(lab >= 0, 0, lab).astype(np.int32), f, 1)
        return o
    out = _ranks(gpu, (2, 2), 50.0, parts, body, center=CENTER, params=params)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
        assert _same_t(o["s"], out[0]["s"]) and _same_t(o["h"], out[0]["h"]) and _same_t(o["k1"], out[0]["k1"]) and o["wide"] and o["dev"], r
    # a kernel that forgets `- own_first` cannot pass: the own points of the higher ranks do not start the local cloud
    halo = 2.0 * float(np.float32(GROUP["graph_size"])) + float(np.float32(GROUP["voxel_size"]))   # (the driver's: its parameters are floats)
    first = [_own_first(parts, r, (2, 2), 50.0, CENTER, halo) for r in range(4)]
    assert first[0] == 0 and all(n > 0 for n in first[1:])
    assert all(out[r]["n_local"] >= first[r] + parts[r].shape[0] for r in range(4))
    assert out[3]["n_local"] == first[3] + parts[3].shape[0]        # the highest rank: lower ranks' strips, then its own points, nothing behind
    K = K_DESIGNED
    lab, field, cls = np.concatenate(labs), np.concatenate(F[5]), np.concatenate(CL[16])
    n_points = out[0]["n_points"]
    assert np.array_equal(n_points, np.bincount(lab[lab >= 0], minlength=K))
    s, h = out[0]["s"], out[0]["h"]
    assert s["n_skipped"] == 0 and h["n_skipped"] == 0
    _check_fields(_sk(s), field, lab, K, n_points)
    _check_hist(_sk(h), cls, lab, K, 16, n_points)
    _check_fields(_sk(out[0]["k1"]), field, np.where(lab >= 0, 0, lab), 1, np.array([(lab >= 0).sum()]))
    _check_own_and_fold(gpu, out, labs, [np.ones(p.shape[0], bool) for p in parts], K, F, CL, {5: _sk(s)}, {16: _sk(h)})
    for r in range(4):
        assert n_points[10 + 5 * r:15 + 5 * r].tolist() == list(SIZES)
        assert np.array_equal(s["n_valid"][10 + 5 * r:15 + 5 * r, 0], np.array(SIZES))
        assert out[r]["pay"]["own_records"] == np.unique(labs[r][labs[r] >= 0]).size
    # a label whose only points on a rank are another rank's halo points: that rank sends no record for it.  Label 1 lives in the left
    # half of a voxel that ranks 0 and 1 share, so rank 1's context holds its points -- as halo
    own1 = out[1]["own"][5]["label"]
    assert 1 not in own1.tolist() and 1 in out[0]["own"][5]["label"].tolist() and 2 in own1.tolist()
    assert out[1]["n_local"] > parts[1].shape[0]
    # labels 15 .. 19 and 25 .. 29: on one rank only, the highest included
    assert all(set(range(10 + 5 * r, 15 + 5 * r)) <= set(out[r]["own"][5]["label"].tolist()) for r in range(4))
    assert not any(k in out[r]["own"][5]["label"].tolist() for r in range(3) for k in range(25, 30))
    # label 0, channel 1: rank 0's record is empty there and the anchor is rank 1's
    o0, o1 = out[0]["own"][5], out[1]["own"][5]
    i0, i1 = int(np.nonzero(o0["label"] == 0)[0][0]), int(np.nonzero(o1["label"] == 0)[0][0])
    assert o0["n_valid"][i0, 1] == 0 and o0["anchor"][i0, 1] == 0 and o0["s1"][i0, 1] == 0 and o0["s2"][i0, 1] == 0
    assert o0["vmin"][i0, 1] == np.inf and o0["vmax"][i0, 1] == -np.inf and o0["n_valid"][i0, 0] > 0
    assert s["n_valid"][0, 1] == o1["n_valid"][i1, 1] > 0 and s["anchor"][0, 1] == o1["anchor"][i1, 1]
    assert s["anchor"][0, 0] == o0["anchor"][i0, 0]
    # label 6, channel 2: invalid everywhere
    assert s["n_valid"][6, 2] == 0 and s["anchor"][6, 2] == 0 and all(np.isnan(s[k][6, 2]) for k in ("mean", "var", "vmin", "vmax"))
    assert s["n_valid"][6, 0] == n_points[6] > 0
    # label 8: one point on each of two ranks
    assert n_points[8] == 2 and (s["n_valid"][8] == 2).all() and (s["vmin"][8] <= s["vmax"][8]).all()
    assert n_points[9] == 0 and (n_points[30:] == 0).all()
    # labels 3 / 4 and 6 / 7 alternate inside voxels that ranks share; the corner voxel holds points of four ranks
    assert n_points[3] > 0 and n_points[4] > 0 and n_points[7] > 0
    assert len(BIG_NODES) > 8


# ---------------------------------------------------------------- 5. general floats
def test_general_floats_within_the_summation_bound(gpu):
    """normal(100, 7) with NaN sprinkled, on 2x2 with two labels inside every voxel, against math.fsum about the table's anchor a within
    the bound of test_gpu_tiles_segfields.test_general_floats_within_the_summation_bound, restated.  u = 2^-52.  Rank r sums its n_r own
    valid values about its own anchor a_r, d = x - a_r (exact): |S1_r - S1x_r| <= e1_r = n_r u sum|d| and |S2_r - S2x_r| <= e2_r = n_r u
    sum d^2 (the chunk sums, their butterflies and the fold of the partials are n_r - 1 additions in some tree).  The fold moves the sums
    to a by delta_r = a_r - a (exact: both are floats' values or 0) with three roundings per rank for S1 and eight for S2, majorised by
    M1 = sum_r (A1_r + n_r |delta_r|) and M2 = sum_r (A2_r + 2 |delta_r| A1_r + n_r delta_r^2):
        E1 = sum_r e1_r + (4 + R) u M1          E2 = sum_r (e2_r + 2 |delta_r| e1_r) + (8 + R) u M2
    and mean and var carry E1 and E2 as that test carries them."""
    tiles = (2, 2)
    parts = _parts(gpu, tiles, n_per=N_PER)
    off = _offsets(parts)
    world = len(parts)
    rng = np.random.default_rng(71)
    G = []
    for p in parts:
        f = rng.normal(100.0, 7.0, (p.shape[0], 2)).astype(np.float32)
        f.reshape(-1)[rng.choice(f.size, f.size // 20, replace=False)] = np.nan
        G.append(f)

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        pl, kept = t.point_labels()
        K = 2 * kept
        lab = _mixed_labels(pl, off[r], 0)
        return dict(K=K, lab=lab, s=t.label_field_stats(lab, G[r], K), own=t.own_point_label_field_moments(K, lab, G[r]))
    out = _ranks(gpu, tiles, _pitch(N_PER), parts, body)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
        assert _same_t(o["s"], out[0]["s"])
    K, got = out[0]["K"], out[0]["s"]
    labels = np.concatenate([o["lab"] for o in out])
    rank_of = np.repeat(np.arange(world), [p.shape[0] for p in parts])
    order = np.argsort(labels, kind="stable")          # stable, and the gathered order is rank order: a label's ranks are runs
    start = np.searchsorted(labels[order], np.arange(K + 1))
    lab_s, rank_s = labels[order], rank_of[order]
    x = np.concatenate(G)[order].astype(np.float64)
    own_a = np.zeros((world, K, 2))
    own_n = np.zeros((world, K, 2), np.int64)
    for r in range(world):
        own_a[r, out[r]["own"]["label"]], own_n[r, out[r]["own"]["label"]] = out[r]["own"]["anchor"], out[r]["own"]["n_valid"]
    fs = lambda v: math.fsum(v.tolist())   # noqa: E731
    worst_m = worst_v = 0.0
    checked = two_ranks = 0
    for k in range(K):
        s0, s1 = int(start[k]), int(start[k + 1])
        if s1 == s0:
            assert (got["n_valid"][k] == 0).all()
            continue
        cut = s0 + np.searchsorted(rank_s[s0:s1], np.arange(world + 1))
        for c in range(2):
            a = got["anchor"][k, c]
            xs = x[s0:s1, c]
            ok = np.isfinite(xs)
            n = int(ok.sum())
            assert n == got["n_valid"][k, c]
            if n == 0:
                continue
            dd = xs[ok] - a
            p, e = _exact_square_parts(dd)
            s1x, s2x = fs(dd), math.fsum(p.tolist() + e.tolist())
            E1 = E2 = M1 = M2 = 0.0
            R = 0
            for r in range(world):
                xr = x[int(cut[r]):int(cut[r + 1]), c]
                xr = xr[np.isfinite(xr)]
                nr = xr.size
                assert nr == own_n[r, k, c]
                if nr == 0:
                    continue
                R += 1
                dr = xr - own_a[r, k, c]
                pr, er = _exact_square_parts(dr)
                A1, A2, dl = fs(np.abs(dr)), math.fsum(pr.tolist() + er.tolist()), abs(own_a[r, k, c] - a)
                e1r, e2r = nr * U * A1, nr * U * A2
                E1 += e1r
                E2 += e2r + 2 * dl * e1r
                M1 += A1 + nr * dl
                M2 += A2 + 2 * dl * A1 + nr * dl * dl
            E1 += (4 + R) * U * M1
            E2 += (8 + R) * U * M2
            two_ranks += R >= 2
            m1x = s1x / n
            meanx, varx = a + m1x, max(0.0, s2x / n - m1x * m1x)
            tol_mean = E1 / n + 2 * U * (abs(m1x) + abs(meanx))
            tol_var = E2 / n + 2 * abs(m1x) * E1 / n + 4 * U * (s2x / n + m1x * m1x)
            em, ev = abs(got["mean"][k, c] - meanx), abs(got["var"][k, c] - varx)
            assert em <= tol_mean, (k, c, n, em, tol_mean)
            assert ev <= tol_var, (k, c, n, ev, tol_var)
            checked += 1
            if tol_mean > 0:
                worst_m = max(worst_m, em / tol_mean)
            if tol_var > 0:
                worst_v = max(worst_v, ev / tol_var)
    assert checked > 100 and two_ranks > 0
    print(f"2x2: {checked} (label, channel) entries, {two_ranks} over two ranks or more; largest mean error / bound = {worst_m:.3g}, "
          f"largest var error / bound = {worst_v:.3g}")


# ---------------------------------------------------------------- 6. the status contract
def test_before_a_run_and_on_the_wrong_kind_of_context(gpu):
    from vgs_svgs_segmentation_amd import tiles_native as tn
    grp = tn.LocalGroup(2)
    t = tn.NativeTiles(gpu.default_params(2, voxel_size=0.1), tn.COMM_LOCAL, grp.handle, 0, 2, (2, 1), 5.0)
    lab, f = np.zeros(4, np.int32), np.zeros((4, 2), np.float32)
    try:
        for call in (lambda: t.label_field_stats(lab, f, 3), lambda: t.label_class_histogram(lab, lab, 3, 3)):
            with pytest.raises(gpu.VgsError) as e:
                call()   # rank 0 alone comes back: no collective
            assert e.value.status == gpu._lib.VGS_E_STATE and "vgs_tiles_run first" in str(e.value)
        for call in (lambda: t.own_point_label_field_moments(3, lab, f), lambda: t.own_point_label_class_counts(3, lab, lab, 3)):
            with pytest.raises(gpu.VgsError) as e:
                call()
            assert e.value.status == gpu._lib.VGS_E_STATE
    finally:
        t.close()
        grp.close()
    # the own-record calls are for tile contexts only
    xyz = gpu.scenes.town_scene(60_000)
    eng = gpu.Engine(gpu.default_params(2))
    eng.set_points(xyz)
    eng.run()
    n = xyz.shape[0]
    lab, f = np.zeros(n, np.int32), np.zeros((n, 2), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n_rec, n_skip = C.c_int64(0), C.c_int64(0)
    st = eng._L.vgs_own_point_label_field_moments(eng._h, 3, p(lab), p(f), n, 2, 8, C.byref(n_rec), C.byref(n_skip), *([None] * 7))
    assert st == gpu._lib.VGS_E_STATE and b"tile context" in eng._L.vgs_last_error_string(eng._h)
    st = eng._L.vgs_own_point_label_class_counts(eng._h, 3, p(lab), p(lab), n, 3, C.byref(n_rec), C.byref(n_skip), None, None, None)
    assert st == gpu._lib.VGS_E_STATE and b"tile context" in eng._L.vgs_last_error_string(eng._h)


def test_failures_travel_in_the_status_word(gpu):
    parts = _parts(gpu, (2, 1), n_per=20_000)

    def attempt(call):
        try:
            return call()
        except Exception as ex:  # noqa: BLE001
            return ex

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        n = xyz.shape[0]
        good = np.zeros(n, np.int32)
        good[-1] = -1
        bad = good.copy()
        if r == 1:
            bad[[700, 311]] = 3
        f, c = _int_field(n, 3, 5 + r), np.zeros(n, np.int32)
        res = {}
        res["label"] = attempt(lambda: t.label_field_stats(bad, f, 3))
        res["label_hist"] = attempt(lambda: t.label_class_histogram(bad, c, 4, 3))
        res["n"] = attempt(lambda: t.label_field_stats(good[:n - (r == 1)], f[:n - (r == 1)], 3))
        res["n_hist"] = attempt(lambda: t.label_class_histogram(good[:n - (r == 1)], c[:n - (r == 1)], 4, 3))
        res["K"] = attempt(lambda: t.label_field_stats(good, f, 3 + r))
        res["K_hist"] = attempt(lambda: t.label_class_histogram(good, c, 4, 3 + r))
        res["channels"] = attempt(lambda: t.label_field_stats(good, _int_field(n, 3 + r, 1), 3))
        res["classes"] = attempt(lambda: t.label_class_histogram(good, c, 4 + r, 3))
        res["big"] = attempt(lambda: t.label_class_histogram(good, c, 1024, (1 << 17) + 1))
        res["big_fields"] = attempt(lambda: t.label_field_stats(good, _int_field(n, 64, 1), (1 << 21) + 1))
        # K = 0 (every label must be negative then): a collective all the same, nothing is written, n_skipped the sum over the ranks, 0
        zero = np.full(n, -1, np.int32)
        res["K0"] = attempt(lambda: t.label_field_stats(zero, f, 0))
        res["K0_hist"] = attempt(lambda: t.label_class_histogram(zero, c, 4, 0))
        res["after"] = attempt(lambda: t.label_field_stats(good, f, 3))   # the driver is usable after all of them
        L, h = gpu._lib.lib(), t._ctx()
        m = t.counts()["points"]
        lab_m, f_m = np.zeros(m, np.int32), np.zeros((m, 2), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        st = L.vgs_point_label_field_stats(h, p(lab_m), 3, p(f_m), m, 2, 8, *([None] * 7))
        msg = L.vgs_last_error_string(h).decode()
        st2 = L.vgs_point_label_class_histogram(h, p(lab_m), 3, p(lab_m), m, 3, *([None] * 5))
        res["single"] = (st, msg, st2)
        return res
    out = _ranks(gpu, (2, 1), _pitch(20_000), parts, body, timeout=120.0)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    E, L = gpu.VgsError, gpu._lib
    for case in ("label", "label_hist"):
        assert isinstance(out[1][case], E) and out[1][case].status == L.VGS_E_ARG and "[311] = 3" in str(out[1][case]), (case, out[1][case])
        assert isinstance(out[0][case], E) and out[0][case].status == L.VGS_E_PEER and "rank 1" in str(out[0][case]), (case, out[0][case])
    for case in ("n", "n_hist"):
        assert isinstance(out[1][case], E) and out[1][case].status == L.VGS_E_ARG and "n_own" in str(out[1][case]), (case, out[1][case])
        assert isinstance(out[0][case], E) and out[0][case].status == L.VGS_E_PEER and "rank 1" in str(out[0][case]), (case, out[0][case])
    for o in out:
        for case in ("K", "K_hist"):
            assert isinstance(o[case], E) and o[case].status == L.VGS_E_ARG and "rank 1 passed K = 4" in str(o[case]), (case, o[case])
        assert isinstance(o["channels"], E) and o["channels"].status == L.VGS_E_ARG and "rank 1 passed n_channels = 4" in str(o["channels"])
        assert isinstance(o["classes"], E) and o["classes"].status == L.VGS_E_ARG and "rank 1 passed n_classes = 5" in str(o["classes"])
        for case in ("big", "big_fields"):
            assert isinstance(o[case], E) and o[case].status == L.VGS_E_UNSUPPORTED and "2^27" in str(o[case]), (case, o[case])
        assert not isinstance(o["K0"], Exception) and all(o["K0"][k].shape == (0, 3) for k in STAT_KEYS) and o["K0"]["n_skipped"] == 0
        assert not isinstance(o["K0_hist"], Exception) and o["K0_hist"]["hist"].shape == (0, 4) and o["K0_hist"]["majority"].shape == (0,)
        assert not isinstance(o["after"], Exception) and _same_t(o["after"], out[0]["after"]), o["after"]
        assert o["single"][0] == L.VGS_E_STATE and "tile context" in o["single"][1] and "vgs_tiles_point_label_field_stats" in o["single"][1]
        assert o["single"][2] == L.VGS_E_STATE


def test_n_skipped_is_the_sum_over_the_ranks_and_K_zero_writes_nothing(gpu):
    parts = _parts(gpu, (2, 1), n_per=20_000)
    bad = np.array([[np.nan, 1.0, 1.0]], np.float32)
    parts = [np.concatenate([p, bad] + ([bad] if r == 1 else [])) for r, p in enumerate(parts)]   # one and two points outside the octree

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        n = xyz.shape[0]
        lab = np.full(n, -1, np.int32)
        lab[-(1 + r):] = 0          # only the points outside the octree carry a label
        neg = np.full(n, -1, np.int32)
        f, c = _int_field(n, 2, r), np.zeros(n, np.int32)
        out = dict(zero=t.label_field_stats(neg, f, 0), zero_h=t.label_class_histogram(neg, c, 4, 0))
        out["one"] = t.label_field_stats(lab, f, 1)       # K = 1: the three points outside the octree are skipped, the row is empty
        out["one_h"] = t.label_class_histogram(lab, c, 4, 1)
        return out
    out = _ranks(gpu, (2, 1), _pitch(20_000), parts, body, timeout=120.0)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
        assert o["zero"]["n_skipped"] == 0 and o["zero"]["mean"].shape == (0, 2) and o["zero_h"]["n_skipped"] == 0 and o["zero_h"]["hist"].shape == (0, 4)
        assert o["one"]["n_skipped"] == 3 and o["one_h"]["n_skipped"] == 3
        assert (o["one"]["n_valid"] == 0).all() and np.isnan(o["one"]["mean"]).all() and o["one_h"]["majority"].tolist() == [-1]


def test_an_injected_failure_takes_the_peer_out(gpu, monkeypatch):
    monkeypatch.setenv("VGS_TILES_FAIL_RANK", "1")
    monkeypatch.setenv("VGS_TILES_FAIL_AT", "point_labels")
    parts = _parts(gpu, (2, 1), n_per=20_000)

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        n = xyz.shape[0]
        errs = []
        for call in (lambda: t.label_field_stats(np.zeros(n, np.int32), _int_field(n, 2, 1), 2),
                     lambda: t.label_class_histogram(np.zeros(n, np.int32), np.zeros(n, np.int32), 4, 2)):
            try:
                call()
                errs.append(None)
            except Exception as ex:  # noqa: BLE001
                errs.append(ex)
        return errs
    out = _ranks(gpu, (2, 1), _pitch(20_000), parts, body, timeout=120.0)
    for r, o in enumerate(out):
        assert not isinstance(o, Exception), (r, o)
    for e in out[1]:
        assert isinstance(e, gpu.VgsError) and e.status == gpu._lib.VGS_E_STATE and "point_labels" in str(e), e
    for e in out[0]:
        assert isinstance(e, gpu.VgsError) and e.status == gpu._lib.VGS_E_PEER and "rank 1" in str(e), e


# ---------------------------------------------------------------- 7. the front end
def test_tiles_run_front_end_writes_the_refined_attribute_tables(gpu, tmp_path):
    tiles = (2, 1)
    parts = _parts(gpu, tiles, n_per=N_PER)
    F, CL = _fields(parts, (5,)), _classes(parts, (16,))
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    prefix = str(tmp_path / "t")
    for r, p in enumerate(parts):
        np.ascontiguousarray(p, dtype=np.float32).tofile(f"{prefix}.{r}.f32")
        F[5][r].tofile(f"{prefix}.{r}.fields.f32")
        CL[16][r].tofile(f"{prefix}.{r}.classes.i32")
    fcsv, ccsv = str(tmp_path / "fields.csv"), str(tmp_path / "classes.csv")
    text = subprocess.check_output([EXE, "--emulate", "2x1", "--pitch", repr(float(_pitch(N_PER))), "--voxel", "0.1", "--refine",
                                    "--refined-segment-fields", fcsv, "--field-channels", "5", "--refined-segment-classes", ccsv, "--classes", "16",
                                    prefix], text=True, timeout=300)
    kept = int(text.strip().splitlines()[0].split()[1])

    def body(r, t, xyz):
        t.set_points(xyz)
        t.run()
        _, k = t.point_labels()
        t.refine_labels()
        fine = t.refined_labels().copy()
        return dict(kept=k, fine=fine, s=t.label_field_stats(fine, F[5][r], k), h=t.label_class_histogram(fine, CL[16][r], 16, k))
    o = _ranks(gpu, tiles, _pitch(N_PER), parts, body)[0]
    assert not isinstance(o, Exception), o
    assert o["kept"] == kept
    assert np.array_equal(np.fromfile(f"{prefix}.0.refined.i32", dtype=np.int32), o["fine"])   # the labels the tables describe
    s, h = o["s"], o["h"]
    with open(fcsv) as f:
        assert f.readline().strip().split(",")[:6] == ["label", "f0_n_valid", "f0_mean", "f0_var", "f0_min", "f0_max"]
    tab = np.loadtxt(fcsv, delimiter=",", skiprows=1, ndmin=2)
    assert tab.shape == (kept, 1 + 5 * 5) and np.array_equal(tab[:, 0], np.arange(kept))
    for c in range(5):
        cols = tab[:, 1 + 5 * c:6 + 5 * c]
        assert np.array_equal(cols[:, 0].astype(np.int64), s["n_valid"][:, c])
        assert np.array_equal(cols[:, 1], s["mean"][:, c], equal_nan=True) and np.array_equal(cols[:, 2], s["var"][:, c], equal_nan=True)
        assert np.array_equal(cols[:, 3].astype(np.float32), s["vmin"][:, c], equal_nan=True)
        assert np.array_equal(cols[:, 4].astype(np.float32), s["vmax"][:, c], equal_nan=True)
    tab = np.loadtxt(ccsv, delimiter=",", skiprows=1, ndmin=2).astype(np.int64)
    assert tab.shape == (kept, 4 + 16) and np.array_equal(tab[:, 0], np.arange(kept))
    assert np.array_equal(tab[:, 1], h["majority"]) and np.array_equal(tab[:, 2], h["majority_count"]) and np.array_equal(tab[:, 3], h["n_outside"])
    assert np.array_equal(tab[:, 4:], h["hist"])
