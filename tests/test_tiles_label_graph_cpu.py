"""CPU tests of the host fold of the adjacency graph of a point labelling across the ranks of the tiled driver
(vgs_tiles_fold_label_edges, include/vgs_tiles.h; tiles_native.fold_label_edges) against a short restatement in Python, and of the front
end's refusals (examples/vgs_tiles_run.cpp), which come before any GPU call.

A rank's partial table: edges (a < b) in strictly ascending order with n_shared, n_pairs, n_finite, nodes_a, nodes_b, w_sum, w_min,
w_max.  The fold merges by (a, b), ranks in ascending order: the counts add, w_sum adds in fp64 in rank order, the extrema come from the
ranks with n_finite > 0 (NaN when there is none)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")
FIELDS = (("seg_ab", np.int32, 2), ("n_shared", np.int64, 1), ("n_pairs", np.int64, 1), ("n_finite", np.int64, 1), ("nodes_ab", np.int32, 2),
          ("w_sum", np.float64, 1), ("w_min", np.float32, 1), ("w_max", np.float32, 1))


@pytest.fixture(scope="module")
def tn(vgs):
    from vgs_svgs_segmentation_amd import tiles_native
    tiles_native.lib()
    return tiles_native


def table(rows):
    """rows: (a, b, n_shared, n_pairs, n_finite, nodes_a, nodes_b, w_sum, w_min, w_max)"""
    rows = list(rows)
    col = lambda i, dt: np.array([r[i] for r in rows], dtype=dt)   # noqa: E731
    return dict(seg_ab=np.array([[r[0], r[1]] for r in rows], dtype=np.int32).reshape(-1, 2), n_shared=col(2, np.int64), n_pairs=col(3, np.int64),
                n_finite=col(4, np.int64), nodes_ab=np.array([[r[5], r[6]] for r in rows], dtype=np.int32).reshape(-1, 2), w_sum=col(7, np.float64),
                w_min=col(8, np.float32), w_max=col(9, np.float32))


def ref_fold(records):
    """the twenty-line restatement"""
    acc = {}
    for R in records:                      # ranks in ascending order
        for i in range(R["seg_ab"].shape[0]):
            key = (int(R["seg_ab"][i, 0]), int(R["seg_ab"][i, 1]))
            e = acc.setdefault(key, dict(ns=0, np_=0, nf=0, na=0, nb=0, ws=np.float64(0.0), mn=None, mx=None))
            e["ns"] += int(R["n_shared"][i]); e["np_"] += int(R["n_pairs"][i]); e["nf"] += int(R["n_finite"][i])
            e["na"] += int(R["nodes_ab"][i, 0]); e["nb"] += int(R["nodes_ab"][i, 1])
            e["ws"] = e["ws"] + np.float64(R["w_sum"][i])
            if R["n_finite"][i] > 0:
                e["mn"] = R["w_min"][i] if e["mn"] is None else min(e["mn"], R["w_min"][i])
                e["mx"] = R["w_max"][i] if e["mx"] is None else max(e["mx"], R["w_max"][i])
    nan = np.float32(np.nan)
    return table((a, b, e["ns"], e["np_"], e["nf"], e["na"], e["nb"], e["ws"], nan if e["mn"] is None else e["mn"], nan if e["mx"] is None else e["mx"])
                 for (a, b), e in sorted(acc.items()))


def same(got, want):
    return all(got[n].dtype == dt and got[n].shape == want[n].shape and got[n].tobytes() == want[n].tobytes() for n, dt, _ in FIELDS)


NAN, INF = float("nan"), float("inf")


def test_designed_edges(tn):
    """an edge on one, on two and on all ranks; one without a finite weight anywhere; one with proxy contributions only on a rank"""
    r0 = table([(0, 1, 1, 4, 3, 2, 2, 1.25, 0.25, 0.5), (0, 2, 0, 2, 0, 1, 1, 0.0, INF, -INF), (1, 3, 2, 7, 7, 3, 4, 3.5, 0.125, 0.75)])
    r1 = table([(0, 1, 0, 1, 1, 1, 1, 0.1, 0.1, 0.1), (0, 2, 0, 1, 0, 1, 0, 0.0, INF, -INF), (2, 3, 0, 5, 2, 2, 2, 0.7, 0.3, 0.4)])
    r2 = table([(0, 1, 0, 0, 0, 1, 0, 0.0, INF, -INF), (1, 3, 0, 1, 1, 0, 1, 0.2, 0.2, 0.2)])   # (0, 1): n_pairs = 0, a proxy's vertex only
    got = tn.fold_label_edges([r0, r1, r2], 4)
    want = ref_fold([r0, r1, r2])
    assert got["n_edges"] == 4 and same(got, want)
    assert got["seg_ab"].tolist() == [[0, 1], [0, 2], [1, 3], [2, 3]]
    assert got["n_shared"].tolist() == [1, 0, 2, 0] and got["n_pairs"].tolist() == [5, 3, 8, 5] and got["nodes_ab"].tolist() == [[4, 3], [2, 1], [3, 5], [2, 2]]
    assert np.isnan(got["w_min"][1]) and np.isnan(got["w_max"][1]) and got["w_sum"][1] == 0.0
    assert got["w_min"].tolist()[0] == np.float32(0.1) and got["w_max"].tolist()[0] == 0.5            # the rank without a finite weight does not count
    assert got["w_sum"][0] == (np.float64(1.25) + np.float64(0.1)) + np.float64(0.0)                  # rank order
    assert same(tn.fold_label_edges([r0], 4), r0 | dict(w_min=np.where(r0["n_finite"] > 0, r0["w_min"], np.float32(np.nan)),
                                                        w_max=np.where(r0["n_finite"] > 0, r0["w_max"], np.float32(np.nan))))
    empty = tn.fold_label_edges([table([]), table([])], 3)
    assert empty["n_edges"] == 0 and all(empty[n].shape[0] == 0 for n, _, _ in FIELDS)


@pytest.mark.parametrize("seed", range(6))
def test_random_rank_tables(tn, seed):
    rng = np.random.default_rng(100 + seed)
    world, K = int(rng.integers(1, 6)), int(rng.integers(2, 9))
    pairs = [(a, b) for a in range(K) for b in range(a + 1, K)]
    records = []
    for _ in range(world):
        rows = []
        for a, b in pairs:
            if rng.random() < 0.5:
                continue
            nf = int(rng.integers(0, 4))
            w = rng.random(max(nf, 1)).astype(np.float32)
            rows.append((a, b, int(rng.integers(0, 3)), nf + int(rng.integers(0, 3)), nf, int(rng.integers(0, 5)), int(rng.integers(0, 5)),
                         float(w[:nf].astype(np.float64).sum()), float(w[:nf].min()) if nf else INF, float(w[:nf].max()) if nf else -INF))
        records.append(table(rows))
    got = tn.fold_label_edges(records, K)
    want = ref_fold(records)
    assert got["n_edges"] == want["seg_ab"].shape[0] and same(got, want), (got, want)


def test_refusals(tn):
    ok = table([(0, 1, 0, 1, 0, 1, 1, 0.0, INF, -INF), (0, 2, 0, 1, 0, 1, 1, 0.0, INF, -INF)])
    assert tn.fold_label_edges([ok, ok], 3)["n_edges"] == 2
    for bad, K in ((ok, 2),                                                                   # a label outside 0 .. K-1
                   (table([(-1, 1, 0, 1, 0, 1, 1, 0.0, INF, -INF)]), 3),
                   (table([(1, 1, 0, 1, 0, 1, 1, 0.0, INF, -INF)]), 3),                        # a >= b
                   (table([(2, 1, 0, 1, 0, 1, 1, 0.0, INF, -INF)]), 3),
                   (table([(0, 2, 0, 1, 0, 1, 1, 0.0, INF, -INF), (0, 1, 0, 1, 0, 1, 1, 0.0, INF, -INF)]), 3),   # not ascending
                   (table([(0, 1, 0, 1, 0, 1, 1, 0.0, INF, -INF), (0, 1, 0, 1, 0, 1, 1, 0.0, INF, -INF)]), 3)):  # not strictly
        with pytest.raises(tn.VgsError, match="VGS_E_ARG"):
            tn.fold_label_edges([ok, bad], K)


def _run(tmp_path, opts):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    return subprocess.run([EXE, "--emulate", "2x1", *opts, str(tmp_path / "t")], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("opts,word", [(["--refined-graph", "a.csv"], "--refined-graph needs --refine"),
                                       (["--class-graph", "b.csv"], "--class-graph needs --classes"),
                                       (["--class-graph", "b.csv", "--classes", "0"], "--classes must be in 1 .. 1024"),
                                       (["--class-graph", "b.csv", "--classes", "2000"], "--classes must be in 1 .. 1024")])
def test_graph_options_are_refused_before_any_gpu_call(tmp_path, opts, word):
    p = _run(tmp_path, opts)
    assert p.returncode == 2 and word in p.stderr and "usage:" in p.stderr, (p.returncode, p.stderr)
    assert "--refined-graph" in p.stderr and "--class-graph" in p.stderr
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("opts", [["--refine", "--refined-graph"], ["--classes", "3", "--class-graph"]], ids=["refined", "classes"])
def test_an_unwritable_path_is_refused_before_any_gpu_call(tmp_path, opts):
    p = _run(tmp_path, opts + [str(tmp_path / "no_such_dir" / "g.csv")])
    assert p.returncode == 2 and "cannot write" in p.stderr and "g.csv" in p.stderr, (p.returncode, p.stderr)
    assert not os.listdir(tmp_path)
