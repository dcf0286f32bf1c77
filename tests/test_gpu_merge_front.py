"""The merge front (k_cross, k_union_mutual) compacts each row's set entries into a list in LDS before it looks anything up.  Nothing
observable may move: the mutual flags are a pure function of the two connect rows, csize is a count, the first hook a minimum and the
union-find's result canonical.  So every case here is compared with the CPU oracle run with the same parameters -- connect_cross and
connect_final as sets per voxel, node labels up to renaming, point labels as they are -- and a second run() and a second Engine must
repeat the arrays.

What the scenes hold was checked with the oracle (lean flavour); connect-list lengths are per used voxel:
  urban_400k   lists of 1 .. 291 voxels: 459 rows with <= 1 (the "list is {self}" branch), 4768 above 32 (more than one trip of the
               dense pass), 597 above 64, 169 above 128; mutual lists up to 176 (the union pass's list
               holds 64, so those rows drain in rounds); and rows are put off at this size, so the second pass over the work list runs
  pc_60k       rows of up to 826 neighbours, median list 205, max 316; 1920 of 2413 used voxels above 128 and most above 256: the
               lists of both kernels (256 and 64 entries) are filled and drained several times per row; 6 rows with <= 1
  noisy_100k   lists up to 102; the "many hand-overs" route: the first pass returns at its gate, k_merge_init runs again and one plain
               pass takes every row
  urban_400k_no_connbits   the first scene with the lattice lookup off: the group-table / binary-search branch runs in the dense pass
and one tiled case (two contexts with owned regions) for the ownership tests of both kernels."""
import os

import numpy as np
import pytest

from helpers import canonical_labels, oracle_params, ragged_sets
from test_gpu_tiles import _run_tiled, _single

pytestmark = pytest.mark.gpu

CASES = [
    # name, scene, n, parameters, knob set around the engine's creation
    ("urban_400k", "urban", 400_000, dict(voxel_size=0.1), None),
    ("pc_60k", "pc", 60_000, dict(voxel_size=0.05, graph_size=0.5), None),
    ("noisy_100k", "noisy", 100_000, dict(voxel_size=0.1), None),
    ("urban_400k_no_connbits", "urban", 400_000, dict(voxel_size=0.1), "VGS_NO_CONNBITS"),
]

_clouds, _refs = {}, {}


def _cloud(gpu, kind, n):
    if (kind, n) not in _clouds:
        sc = gpu.scenes
        _clouds[kind, n] = {"urban": sc.urban_scene, "pc": sc.pc_scene, "noisy": sc.noisy_surface_scene}[kind](n)
    return _clouds[kind, n]


def _engine(gpu, p, xyz, knob):
    old = os.environ.get(knob) if knob else None
    if knob:
        os.environ[knob] = "1"
    try:
        eng = gpu.Engine(p)
        eng.set_points(xyz)
        eng.run()
        return eng
    finally:
        if knob:
            if old is None:
                del os.environ[knob]
            else:
                os.environ[knob] = old


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request, gpu, oracle):
    name, kind, n, kw, knob = request.param
    xyz = _cloud(gpu, kind, n)
    p = gpu.default_params(2, **kw)
    eng = _engine(gpu, p, xyz, knob)
    key = (kind, n)   # the knob only chooses the lookup: one oracle run serves both urban cases
    if key not in _refs:
        _refs[key] = oracle.run_vgs(xyz, oracle_params(oracle, p))
    return dict(name=name, xyz=xyz, p=p, eng=eng, ref=_refs[key], knob=knob)


def test_case_reaches_its_path(case):
    eng = case["eng"]
    sc = eng.schedule_counters()
    if case["name"].startswith("urban_400k"):
        assert sc["cross_put_off"] > 0, sc      # the put-off pass with its work list ran
    if case["name"] == "noisy_100k":
        c = eng.counts()
        assert sc["voted_over"] > 0 or c["handed_over"] > 0.5 * c["used"], (sc, c)
    off, _ = case["ref"].lists("connect_cut")
    used = case["ref"].nodes()["used"].astype(bool)
    lens = np.diff(off)[used]
    if case["name"] == "pc_60k":
        assert (lens > 256).sum() > 0 and (lens > 128).sum() > lens.size // 2, (int(lens.max()), int((lens > 128).sum()))
    if case["name"].startswith("urban_400k"):
        assert (lens <= 1).sum() > 0 and (lens > 128).sum() > 0 and (lens > 64).sum() > (lens > 128).sum(), int(lens.max())


@pytest.mark.parametrize("which", ["connect_cross", "connect_final"])
def test_connect_lists_equal_the_oracles(case, which):
    gs, rs = ragged_sets(*case["eng"].lists(which)), ragged_sets(*case["ref"].lists(which))
    bad = [v for v in range(len(rs)) if gs[v] != rs[v]]
    assert not bad, f"{which}: {len(bad)} of {len(rs)} voxels differ, first {bad[:5]}: gpu={sorted(gs[bad[0]])} ref={sorted(rs[bad[0]])}"


def test_labels_equal_the_oracles(case):
    eng, ref = case["eng"], case["ref"]
    pl_ref, nc_ref = ref.labels()
    root, _ = eng.node_labels()
    np.testing.assert_array_equal(canonical_labels(root), canonical_labels(nc_ref))
    np.testing.assert_array_equal(eng.point_labels(), pl_ref)


def _arrays(eng):
    out = [eng.point_labels().copy(), eng.node_labels()[0].copy()]
    for which in ("connect_cross", "connect_final"):
        off, idx = eng.lists(which)
        out += [off.copy(), idx.copy()]
    return out


def test_second_run_and_second_engine_repeat_the_arrays(case, gpu):
    eng = case["eng"]
    first = _arrays(eng)
    eng.run()
    for a, b in zip(first, _arrays(eng)):
        np.testing.assert_array_equal(a, b)
    e2 = _engine(gpu, case["p"], case["xyz"], case["knob"])
    for a, b in zip(first, _arrays(e2)):
        np.testing.assert_array_equal(a, b)


def test_two_owned_regions_label_like_one_engine(gpu):
    """Two contexts with owned regions over a 120 k-point urban scene (the Python twin of the tiled driver, two threads): both kernels
    run their ownership tests.  The partition must be the single engine's, up to the names of the segments."""
    world, n_total = 2, 120_000
    n_per = n_total // world
    pitch = 50.0 * np.sqrt(n_per / 10_000_000)
    parts = [gpu.scenes.tiled_urban_scene(n_total, tiles=(world, 1), tile_index=r) for r in range(world)]
    kw = dict(voxel_size=0.1)
    eng = _single(gpu, np.concatenate(parts), kw)
    out = _run_tiled(gpu, parts, kw, pitch)
    tiled = np.concatenate([out[r][0] for r in range(world)])
    ref = eng.point_labels()
    differ = int((canonical_labels(tiled) != canonical_labels(ref)).sum())
    print(f"tiled against single engine: {differ} of {ref.size} points in differently composed segments; kept {out[0][1]} / {eng.counts()['kept']}")
    assert out[0][1] == out[1][1] == eng.counts()["kept"]
    np.testing.assert_array_equal(canonical_labels(tiled), canonical_labels(ref))
