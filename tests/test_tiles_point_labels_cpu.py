"""CPU tests of the point-labelling tables of the tiled driver: the pair fold (vgs_tiles_fold_label_pairs, csrc/tiles.cpp) against numpy
unique, and the front end's refusal of --refined-* options without --refine (before any GPU call)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")


@pytest.fixture(scope="module")
def tn(vgs):
    from vgs_svgs_segmentation_amd import tiles_native
    tiles_native.lib()
    return tiles_native


def _rec(code, label):
    return {"pair_code": np.asarray(code, dtype=np.uint64), "pair_label": np.asarray(label, dtype=np.int32)}


def _want(records, K):
    code = np.concatenate([r["pair_code"] for r in records]).astype(np.uint64)
    lab = np.concatenate([r["pair_label"] for r in records]).astype(np.int64)
    pairs = np.unique(np.stack([lab.astype(np.uint64), code], axis=1), axis=0) if lab.size else np.zeros((0, 2), np.uint64)
    return np.bincount(pairs[:, 0].astype(np.int64), minlength=K).astype(np.int32)


def test_distinct_pairs_inside_one_rank_and_across_ranks(tn):
    big = (1 << 63) + 12345   # codes use all 64 bits
    records = [_rec([7, 7, 9, big, big], [0, 0, 0, 3, 2]),          # a duplicate inside one rank's list; one code under two labels
               _rec([], []),                                          # an empty rank
               _rec([7, big, 11, 7], [0, 3, 4, 1]),                   # the same pairs again from another rank, and new ones
               _rec([11, 11], [4, 4])]
    K = 6
    got = tn.fold_label_pairs(records, K)
    assert got.dtype == np.int32 and got.tolist() == _want(records, K).tolist() == [2, 1, 1, 1, 1, 0]


def test_random_pairs_match_numpy_unique(tn):
    rng = np.random.default_rng(5)
    K = 37
    records = [_rec(rng.integers(0, 50, n).astype(np.uint64) << np.uint64(40), rng.integers(0, K, n)) for n in (0, 1, 400, 2500)]
    assert np.array_equal(tn.fold_label_pairs(records, K), _want(records, K))
    # the order of the ranks and of the records inside a rank does not matter
    shuffled = [_rec(r["pair_code"][::-1], r["pair_label"][::-1]) for r in records[::-1]]
    assert np.array_equal(tn.fold_label_pairs(shuffled, K), _want(records, K))


def test_a_label_out_of_range_is_refused(tn, vgs):
    for bad in (5, -1):
        with pytest.raises(vgs.VgsError) as e:
            tn.fold_label_pairs([_rec([1, 2], [0, 4]), _rec([3], [bad])], 5)
        assert e.value.status == vgs._lib.VGS_E_ARG


def test_K_zero(tn, vgs):
    assert tn.fold_label_pairs([_rec([], []), _rec([], [])], 0).shape == (0,)
    with pytest.raises(vgs.VgsError) as e:
        tn.fold_label_pairs([_rec([1], [0])], 0)
    assert e.value.status == vgs._lib.VGS_E_ARG


@pytest.mark.parametrize("opts", [["--refined-segments", "a.csv"], ["--refined-segment-boxes", "b.csv"], ["--refined-matches", "c.csv"],
                                  ["--refined-matches", "c.csv", "--refined-truth-matches", "d.csv"], ["--refined-truth-matches", "d.csv"],
                                  ["--patch-radius", "0.1"]])
def test_refined_options_need_refine(tmp_path, opts):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    p = subprocess.run([EXE, "--emulate", "2x1", *opts, str(tmp_path / "t")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "need --refine" in p.stderr, (p.returncode, p.stderr)
    if opts[0].startswith("--refined"):
        assert "usage:" in p.stderr
    assert not os.listdir(tmp_path)
