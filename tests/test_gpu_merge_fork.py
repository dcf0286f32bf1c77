"""The merge stage forks behind crossValidation's first pass: the main stream runs k_compress and the first union pass while a side
stream finishes the local cut, runs crossValidation over the rows put off and closestCheck with its read-backs; the unions of the put-off
rows follow on the main stream beside closestCheck, and the main stream joins before the re-attachment edges.  Every array is computed by the same kernels from the same inputs, so each route is compared
with the CPU oracle run with the same parameters -- connect_cross and connect_final as sets per voxel, node labels up to renaming, point
labels as they are, the numbers of isolated and re-attached voxels -- and the route itself is asserted from the engine's counters, so
that a scene that stops reaching it fails here.

  urban_400k    the forked route with rows put off and closestCheck candidates
  noisy_100k    the hand-overs are many: the first pass and its unions are void, the main stream joins at once and redoes the pass
  plane_40k     no hand-over, no row put off: the fork with an empty side chain in front of closestCheck
  plane_40k_no_overlap   the same cloud with VGS_NO_OVERLAP: the merge stage starts behind the hand-over kernels and takes the path without
                the fork (every run with a used voxel queues hand-over kernels, so this knob is what reaches that path)
  chain         twelve isolated single-voxel candidates in a row beside a patch of parallel sheets, 0.375 m apart with graph_size 0.51:
                each candidate's only eligible neighbour is the candidate before it ("an earlier candidate that succeeded"), so the fixed
                point needs more passes than the four of one round and the second round with its read-back runs

The oracle's counts come from its lists: closestCheck looks at a voxel whose list is {self} after crossValidation and whose adjacency
vector (count + neighbours) is longer than adjacency_min, and a re-attachment appends the target to that list (and the voxel to the
target's); nothing is appended to a list of length one before its own turn, because such a voxel is not an eligible target."""
import numpy as np
import pytest

import cut_order_scenes as cs
from helpers import canonical_labels, oracle_params, ragged_lists, ragged_sets
from test_gpu_merge_front import _cloud, _engine, _refs
from test_gpu_tiles import _run_tiled, _single

pytestmark = pytest.mark.gpu

CHAIN_LINKS = 12


def plane_scene(n=40_000, seed=5):
    """A clean 2 m x 2 m plane, 100 points per 0.1 m voxel: nothing for the lazy schedule to give up on."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0.0, 2.0, (n, 3))
    xyz[:, 2] = rng.uniform(-0.002, 0.002, n)
    return xyz.astype(np.float32)


def chain_scene(links=CHAIN_LINKS, seed=0):
    """Sheet voxels (cut_order_scenes) on an exact lattice: a 6 x 6 patch of parallel sheets (they connect with each other) and, towards
    smaller x, `links` single sheets six cells apart whose normals alternate between x and y (90 degrees to each other and to the
    patch's: every local cut returns them alone).  Voxel ids ascend along the row away from the patch."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    patch = np.stack([gx.ravel() + 6 * links, gy.ravel(), np.zeros(36, dtype=np.int64)], axis=1)
    chain = np.stack([6 * np.arange(links)[::-1], np.full(links, 2), np.zeros(links, dtype=np.int64)], axis=1)
    normals = np.where((np.arange(links) % 2 == 0)[:, None], [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    off_c = np.einsum("pij,pj->pi", np.repeat(cs._rotations(normals), cs.PTS, axis=0), cs._sheet_offsets(rng, links * cs.PTS))
    off = np.concatenate([cs._sheet_offsets(rng, 36 * cs.PTS), off_c])
    return cs._place(np.concatenate([patch, chain]), off)


CASES = [
    # name, cloud, parameters, knob set around the engine's creation
    ("urban_400k", ("urban", 400_000), dict(voxel_size=0.1), None),
    ("noisy_100k", ("noisy", 100_000), dict(voxel_size=0.1), None),
    ("plane_40k", ("plane", 40_000), dict(voxel_size=0.1), None),
    ("plane_40k_no_overlap", ("plane", 40_000), dict(voxel_size=0.1), "VGS_NO_OVERLAP"),
    ("chain", ("chain", CHAIN_LINKS), dict(voxel_size=cs.RES, graph_size=0.51, adjacency_min=1, q7_count_as_index=0), None),
]


def _xyz(gpu, key):
    kind, n = key
    if kind == "plane":
        return plane_scene(n)
    if kind == "chain":
        return chain_scene(n)
    return _cloud(gpu, kind, n)


def _oracle_closest_check(ref, adjacency_min):
    """(candidates, re-attached candidates, their targets) of the oracle's closestCheck, from its lists."""
    cross = np.diff(ref.lists("connect_cross")[0])
    adj = np.diff(ref.lists("adjacency")[0])
    final = ragged_lists(*ref.lists("connect_final"))
    used = ref.nodes()["used"].astype(bool)
    cand = np.flatnonzero(used & (cross == 1) & (adj + 1 > adjacency_min))
    succ = [int(v) for v in cand if len(final[v]) > 1]
    return cand, succ, {v: final[v][1] for v in succ}


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request, gpu, oracle):
    name, key, kw, knob = request.param
    xyz = _xyz(gpu, key)
    p = gpu.default_params(2, **kw)
    eng = _engine(gpu, p, xyz, knob)
    if key not in _refs:   # (shared with test_gpu_merge_front's cases: the same clouds and parameters, one oracle run)
        _refs[key] = oracle.run_vgs(xyz, oracle_params(oracle, p))
    return dict(name=name, xyz=xyz, p=p, eng=eng, ref=_refs[key], knob=knob, cc=_oracle_closest_check(_refs[key], p.adjacency_min))


def test_case_reaches_its_route(case):
    eng, name = case["eng"], case["name"]
    sc, c = eng.schedule_counters(), eng.counts()
    cand, succ, target = case["cc"]
    print(f"{name}: schedule {sc}\n{name}: used {c['used']} handed over {c['handed_over']} isolated {c['isolated']} reattached {c['reattached']}")
    if name == "urban_400k":
        assert sc["handed_over"] > 0 and sc["cross_put_off"] > 0, sc       # hand-over kernels, the put-off pass on the side stream
        assert c["isolated"] > 0 and c["reattached"] > 0, c                # closestCheck's candidates, passes and both read-backs
        assert sc["handed_over"] <= c["used"] // 8, (sc, c)                # few: the first pass counts
    if name == "noisy_100k":
        # more hand-overs than an eighth of the used voxels (VGS_PG_MINFRAC's default): k_ho_lists writes LC_MANY
        assert sc["handed_over"] > c["used"] // 8 and sc["pair_list_cut"] > 0, (sc, c)
    if name.startswith("plane_40k"):
        assert c["used"] > 300 and sc["handed_over"] == 0 and sc["handed_over_large"] == 0 and sc["cross_put_off"] == 0, (sc, c)
    if name == "chain":
        # kept only because the oracle shows the chain: every link re-attached, each to the link before it
        chained = [v for v in succ if target[v] in succ]
        assert len(succ) >= 6 and len(chained) >= CHAIN_LINKS - 1, (succ, target)
        assert all(target[v] < v for v in chained)
        assert c["reattached"] >= 6, c


def test_closest_check_counts_equal_the_oracles(case):
    c = case["eng"].counts()
    cand, succ, _ = case["cc"]
    assert (c["isolated"], c["reattached"]) == (len(cand), len(succ))


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
    c = eng.counts()
    return out + [np.array([c[k] for k in ("voxels", "used", "clusters", "kept", "isolated", "reattached", "handed_over")])]


def test_five_runs_and_a_second_engine_repeat_the_arrays(gpu):
    """The main stream's unions and the side chain run at the same time: a race between them would show as an array that moves."""
    xyz = _cloud(gpu, "urban", 400_000)
    p = gpu.default_params(2, voxel_size=0.1)
    eng = _engine(gpu, p, xyz, None)
    first = _arrays(eng)
    assert eng.schedule_counters()["cross_put_off"] > 0 and first[-1][-3] > 0      # the forked route with both side-chain parts
    for _ in range(5):
        eng.run()
        for a, b in zip(first, _arrays(eng)):
            np.testing.assert_array_equal(a, b)
    e2 = _engine(gpu, p, xyz, None)
    for a, b in zip(first, _arrays(e2)):
        np.testing.assert_array_equal(a, b)


def test_two_owned_regions_label_like_one_engine(gpu):
    """Two contexts with owned regions (the Python twin of the tiled driver, two threads): each takes the fork on its own streams."""
    world, n_total = 2, 120_000
    n_per = n_total // world
    pitch = 50.0 * np.sqrt(n_per / 10_000_000)
    parts = [gpu.scenes.tiled_urban_scene(n_total, tiles=(world, 1), tile_index=r) for r in range(world)]
    kw = dict(voxel_size=0.1)
    eng = _single(gpu, np.concatenate(parts), kw)
    out = _run_tiled(gpu, parts, kw, pitch)
    for r in range(world):
        assert out[r][2]["used"] > 0, out[r][2]      # a context with used voxels queues hand-over kernels and forks
    tiled = np.concatenate([out[r][0] for r in range(world)])
    assert out[0][1] == out[1][1] == eng.counts()["kept"]
    np.testing.assert_array_equal(canonical_labels(tiled), canonical_labels(eng.point_labels()))


def test_no_finite_point_returns_as_before(gpu):
    xyz = np.full((100, 3), np.nan, dtype=np.float32)
    xyz[::3, 1] = np.inf
    eng = gpu.Engine(gpu.default_params(2))
    for _ in range(2):
        eng.set_points(xyz)
        eng.run()
        c = eng.counts()
        assert (c["points"], c["finite"], c["voxels"], c["kept"], c["isolated"], c["reattached"]) == (100, 0, 0, 0, 0, 0)
        assert (eng.point_labels() == -1).all()


def test_no_used_voxel_returns_as_before(gpu):
    """U == 0 between two forked runs of one engine: no fork, no side chain left over from the run before, the counters of a fresh engine."""
    sparse = gpu.scenes.urban_scene(21_170, seed=206792296)
    p = gpu.default_params(2, voxel_size=0.08)
    plane = plane_scene()
    eng = gpu.Engine(p)
    eng.set_points(plane); eng.run()
    kept = eng.counts()["kept"]
    labels = eng.point_labels().copy()
    assert kept > 0
    eng.set_points(sparse); eng.run()
    c = eng.counts()
    assert c["used"] == 0 and c["kept"] == 0 and c["clusters"] == c["voxels"] > 0 and c["isolated"] == 0 and c["reattached"] == 0
    assert (eng.point_labels() == -1).all()
    assert not any(eng.schedule_counters().values())
    root, kept_of = eng.node_labels()
    assert (root == np.arange(c["voxels"])).all() and (kept_of == -1).all()
    eng.set_points(plane); eng.run()
    assert eng.counts()["kept"] == kept
    np.testing.assert_array_equal(eng.point_labels(), labels)
