"""The node records of csrc/features.hip (k_features: centroid, normal, eight eigen features, used flag) at the limits of the kernel's
structure and of the eigen solver in csrc/vgs_math.h, on the scenes of tests/attribute_scenes.py: runs that start, end and cross the
edges of the LDS tiles of a workgroup's point range, a voxel of more than three tiles, the partial last workgroup, voxels of one to four
points, and one node per degenerate family of matrices (zero, rank one, rank two, double and triple eigenvalues) near the origin and 149
units out.  Three legs: the CPU oracle's records (the same header compiled for the host), the numpy restatement of
tests/attribute_ref.py (no code of the kernel's loop), both bit for bit, and float64 with np.linalg.eigh within the project's criteria
for the closed-form solver.  tests/test_attribute_ref_cpu.py holds the scenes to what they promise."""
import numpy as np
import pytest

import attribute_ref as R
import attribute_scenes as S
from helpers import canonical_labels, oracle_params, ragged_lists, ragged_sets

pytestmark = pytest.mark.gpu


def _attributes(gpu, sc, eng=None, chain=False):
    """The node records of a scene from an engine (a fresh one unless given): VGS after voxelize + features, SVGS after the caller's labels
    and svgs_segment; chain: VGS goes on through the whole of run()."""
    p = gpu.default_params(sc["method"], **sc["params"])
    if eng is None:
        eng = gpu.Engine(p)
        eng.set_points(sc["xyz"])
    else:
        eng.set_params(p)
    if sc["method"] == 2:
        eng.voxelize()
        eng.features()
        a = eng.attributes()
        if chain:
            eng.run()
            assert _bytes(eng.attributes()) == _bytes(a)
    else:
        eng.set_supervoxel_labels(sc["labels"], sc["max_label"])
        eng.svgs_segment()
        a = eng.attributes()
    return eng, p, a


def _oracle(oracle, sc, p):
    if sc["method"] == 2:
        return oracle.run_vgs(sc["xyz"], oracle_params(oracle, p))
    return oracle.run_svgs_from_labels(sc["xyz"], sc["labels"], sc["max_label"], oracle_params(oracle, p))


def _bytes(a):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in a.items()}


def _same_bits(got, want, what):
    assert np.array_equal(got["used"], want["used"]), what
    for k in ("centroid", "normal", "eigen"):   # as uint32: NaN payloads and the sign of zero count
        bad = np.flatnonzero((got[k].view(np.uint32) != want[k].view(np.uint32)).any(axis=1))
        assert bad.size == 0, f"{what}: {k} of {bad.size} nodes differs, first {bad[:5]}: {got[k][bad[:2]]} against {want[k][bad[:2]]}"


@pytest.fixture(scope="module", params=S.CASES)
def run(request, gpu, oracle):
    sc = S.build(request.param)
    eng, p, a = _attributes(gpu, sc, chain=True)
    ref = _oracle(oracle, sc, p)
    t = eng.voxel_table()
    start, pidx = t["start"].astype(np.int64), t["point_idx"]
    mine = R.nodes_f32(oracle, sc["xyz"], start, pidx, a["used"], sc["method"] == 3)
    return dict(name=request.param, sc=sc, p=p, eng=eng, ref=ref, attrs=a, start=start, pidx=pidx, mine=mine)


def test_table_and_used_flags(run):
    eng, ref, sc = run["eng"], run["ref"], run["sc"]
    c = eng.counts()
    assert c["voxels"] == ref.V
    if sc["method"] == 2:
        r = ref.voxel_table()
        g = eng.voxel_table()
        for k in ("key", "start", "point_idx"):
            np.testing.assert_array_equal(g[k], r[k])
        np.testing.assert_array_equal(eng.point_voxel(), r["point_voxel"])
    else:
        off, idx = ref.lists("sv_points")
        np.testing.assert_array_equal(run["start"], off)
        np.testing.assert_array_equal(run["pidx"], idx)
    np.testing.assert_array_equal(run["attrs"]["used"], ref.nodes()["used"])
    if not run["name"].startswith("degenerate"):
        np.testing.assert_array_equal(np.diff(run["start"]), sc["table"]["sizes"])


def test_records_equal_the_oracle_and_the_restatement_bit_for_bit(run):
    _same_bits(run["attrs"], run["ref"].nodes(), "against the oracle")
    _same_bits(run["attrs"], dict(run["mine"], used=run["attrs"]["used"]), "against the numpy restatement")
    unused = ~run["attrs"]["used"].astype(bool)
    for k in ("centroid", "normal", "eigen"):
        assert (run["attrs"][k][unused].view(np.uint32) == 0).all()     # an unused node's record is all +0.0


def test_float64_leg(run):
    """Centroid and normal are the engine's; the eigenvalues, which the engine does not export, are the restatement's, whose records the
    engine's equal bit for bit.  No row of these scenes is left out (tests/test_attribute_ref_cpu.py asserts the same of the oracle)."""
    sc, a = run["sc"], run["attrs"]
    if run["name"].startswith("degenerate"):
        assert not [r for r in sc["table"] if r["fp64_skip"]]
    bad = R.f64_leg(sc["xyz"], sc["method"] == 3, run["start"], run["pidx"], a["used"], a["centroid"], a["normal"], run["mine"]["evals"])
    assert not bad, bad[:5]


def test_features_within_the_numpy_formulas(run):
    used = run["attrs"]["used"].astype(bool)
    R.check_features(run["attrs"]["eigen"][used], run["mine"]["evals"][used], run["sc"]["method"] == 3)


def test_whole_chain_equals_the_oracle(run):
    """Adjacency, the three connect lists and the labels: where the valid flags of a record (a zero centroid coordinate, a zero normal
    component) and every weight made from it are observed."""
    eng, ref = run["eng"], run["ref"]
    assert ragged_lists(*eng.lists("adjacency")) == ragged_lists(*ref.lists("adjacency"))
    for which in ("connect_cut", "connect_cross", "connect_final"):
        gs, rs = ragged_sets(*eng.lists(which)), ragged_sets(*ref.lists(which))
        bad = [v for v in range(len(rs)) if gs[v] != rs[v]]
        assert not bad, f"{which}: {len(bad)} of {len(rs)} nodes differ, first {bad[:5]}"
    c = eng.counts()
    assert (c["clusters"], c["kept"]) == (ref.clusters_num, ref.kept_clusters)
    pl, nc = ref.labels()
    np.testing.assert_array_equal(canonical_labels(eng.node_labels()[0]), canonical_labels(nc))
    np.testing.assert_array_equal(eng.point_labels(), pl)


def test_points_min_10_0_10_on_one_engine(gpu, oracle):
    sc = S.build("runs_vgs")
    eng, got = None, []
    for pm in (10, 0, 10):
        s = dict(sc, params=dict(sc["params"], points_min=pm))
        eng, p, a = _attributes(gpu, s, eng)
        _same_bits(a, _oracle(oracle, s, p).nodes(), f"points_min {pm}")
        cnt = np.diff(eng.voxel_table()["start"])
        np.testing.assert_array_equal(a["used"].astype(bool), cnt > pm)
        got.append(a)
    assert _bytes(got[2]) == _bytes(got[0]) and _bytes(got[1]) != _bytes(got[0])
    few = np.flatnonzero(cnt <= 3)                                       # used at points_min 0 with the zero matrix
    assert few.size >= 6 and (got[1]["eigen"][few] == 0).all() and not got[0]["used"][few].any()
    n = got[1]["normal"][few]
    assert (np.abs(n[:, 0]) == 1).all() and (n[:, 1:] == 0).all()
    assert np.array_equal(np.signbit(n[:, 1]), np.signbit(n[:, 0])) and np.array_equal(np.signbit(n[:, 2]), np.signbit(n[:, 0]))
    assert np.signbit(n[:, 0]).any()


def test_a_second_fresh_engine_gives_the_same_bytes(run, gpu):
    _, _, a = _attributes(gpu, run["sc"])
    assert _bytes(a) == _bytes(run["attrs"])
