"""The merge stage (csrc/merge.hip) at its structural limits, on the designed scenes of tests/merge_scenes.py whose answer is known in
advance.  One engine run per case is compared three ways, all of them exact:

  1. with the truth by construction: components (roots are smallest ids), kept labels, point labels, the numbers of clusters and kept ones;
  2. with tests/merge_ref.py, the sequential restatement of stages a8-a11, fed with the engine's OWN adjacency rows, local cuts and node
     records: connect_cross and connect_final as sets per voxel, roots, kept labels and point labels as they are, and the counts;
  3. with the CPU oracle end to end, as tests/test_gpu_merge_fork.py does (the clique sizes above 129 leave this leg out: the oracle's
     local cuts cost n^3 per clique).
tests/test_merge_scenes_cpu.py shows on the oracle that every scene reaches the limit it is named for, and prints the figures.

  clique ladder   rows of 1 .. 513 entries, all connected and mutual: on, below and above the list capacities of k_cross and k_union_mutual
  bridges         one union per element that no first hook and no other edge replaces, at list position 62, 63, 64 of its row
  snake           two components of graph diameter 7137 with interleaved ids: long parent chains, k_compress beside the unions, k_flatten
  rods            2500 components of 1 .. 8 voxels, up to 80 distinct roots in a workgroup of k_flatten; voxels_min on either side of the sizes
  count_edges     V on, below and above the workgroups of k_flatten, k_voxel_labels and k_root_flags; voxel V - 1 kept, dropped, no root
  chains, wide_tie, count_as_index, out_of_range   closestCheck's direction rule, tie rule (per lane and across the 64 lanes), candidate
                  test over all neighbours, and the count read as a voxel id, in and out of range
The snake, rods, bridges and closestCheck scenes run through the forked route and, with VGS_NO_OVERLAP, through the path without the fork.

What the scenes are built around, each constant with its kernel:"""
import time

import numpy as np
import pytest

import merge_ref as mr
import merge_scenes as ms
from helpers import canonical_labels, oracle_params, ragged_lists, ragged_sets
from test_gpu_merge_fork import _oracle_closest_check
from test_gpu_merge_front import _engine

pytestmark = pytest.mark.gpu

CX_LIST = 256          # k_cross: 32 lanes per row, MF_CAP_TRIPS 8 -> 256 list positions per round, filled in batches of 4 x 32 flags
UM_LIST = 64           # k_union_mutual: 8 lanes per row -> 64 list positions per round, filled in batches of 8 x 8 flags
FLATTEN_SLOTS = 32     # k_flatten: roots per workgroup table (4 probes), then global atomics
BLOCK = 256            # k_merge_init, k_compress, k_flatten, k_voxel_labels: voxels per workgroup
ROOT_FLAGS_BLOCK = 1024   # k_root_flags: voxels per workgroup, one global atomic each
CC_PASSES = 4          # k_cc_pass<false> launches per closestCheck round, one read-back per round
CC_LANES = 64          # k_cc_pass: lanes that share a candidate's scan

assert {n for c in (UM_LIST, 2 * UM_LIST, CX_LIST, CX_LIST + 2 * UM_LIST, 2 * CX_LIST) for n in (c - 1, c, c + 1)} <= set(ms.LADDER)
assert tuple(m + 1 for m in ms.BRIDGES) == (UM_LIST - 2, UM_LIST - 1, UM_LIST)      # the bridge's list position: the last of a partly
#                                                                                      filled list, of a full one, the first of a second round
assert {n for c in (UM_LIST, BLOCK, ROOT_FLAGS_BLOCK) for n in (c - 1, c, c + 1)} | {2 * ROOT_FLAGS_BLOCK + 1} <= set(ms.COUNT_EDGES)

ROUTES = (None, "VGS_NO_OVERLAP")      # the forked route (default), and the path without the fork
KINDS = ("singles", "last_single", "last_pair")

# name, builder, routes
CASES = [("ladder_oracle", lambda: ms.clique_ladder(ms.LADDER_ORACLE), (None,)), ("bridges", ms.bridges, ROUTES), ("snake", ms.snake, ROUTES)]
CASES += [(f"rods_vm{vm}", (lambda vm=vm: ms.rods(voxels_min=vm)), ROUTES) for vm in ms.VOXELS_MIN]
CASES += [(f"edges_{V}_{k}", (lambda V=V, k=k: ms.count_edges(V, k)), (None,)) for V in ms.COUNT_EDGES for k in KINDS if not (V == 1 and k == "last_pair")]
CASES += [("chains", ms.chains, ROUTES), ("wide_tie", ms.wide_tie, ROUTES)]
CASES += [(f"q7_{q7}_am{am}", (lambda q7=q7, am=am: ms.count_as_index(q7, am)), ROUTES) for q7 in (0, 1) for am in (1, 3, 4)]
CASES += [(f"out_of_range_{n}", (lambda n=n: ms.count_as_index_out_of_range(n)), ROUTES) for n in (2, 3, 4, 5)]
PARAMS = [(name, build, knob) for name, build, routes in CASES for knob in routes]

_scenes, _oracle_runs = {}, {}


def _scene(name, build):
    if name not in _scenes:
        _scenes[name] = build()
    return _scenes[name]


def _restate(oracle, eng, p):
    nodes = eng.attributes()
    return mr.merge_stage(nodes["used"], ragged_lists(*eng.lists("adjacency")), ragged_lists(*eng.lists("connect_cut")),
                          mr.oracle_weight(oracle, nodes, oracle_params(oracle, p)), p.adjacency_min, p.q7_count_as_index, p.voxels_min,
                          eng.point_voxel())


@pytest.fixture(scope="module", params=PARAMS, ids=[f"{n}-{k or 'fork'}" for n, _, k in PARAMS])
def case(request, gpu, oracle):
    name, build, knob = request.param
    sc = _scene(name, build)
    p = gpu.default_params(2, **sc["params"])
    t0 = time.perf_counter()
    eng = _engine(gpu, p, sc["xyz"], knob)
    t_run = time.perf_counter() - t0
    if name not in _oracle_runs:
        _oracle_runs[name] = oracle.run_vgs(sc["xyz"], oracle_params(oracle, p, threads=16))
    c = eng.counts()
    print(f"{name} [{knob or 'fork'}]: {c['voxels']} voxels, used {c['used']}, clusters {c['clusters']}, kept {c['kept']}, isolated {c['isolated']}, "
          f"re-attached {c['reattached']}; create + set_points + run {t_run * 1e3:.0f} ms")
    return dict(name=name, sc=sc, p=p, eng=eng, knob=knob, ref=_oracle_runs[name], truth=ms.truth(sc, eng.point_voxel()))


def _check_truth(sc, eng, t=None):
    t = t or ms.truth(sc, eng.point_voxel())
    root, kept = eng.node_labels()
    np.testing.assert_array_equal(root, t["root"])
    np.testing.assert_array_equal(kept, t["kept"])
    np.testing.assert_array_equal(eng.point_labels(), t["point_labels"])
    c = eng.counts()
    assert (c["voxels"], c["clusters"], c["kept"]) == (sc["cells"].shape[0], t["clusters"], t["n_kept"])
    assert eng.schedule_counters()["outside_limits"] == 0
    return t


def _check_restatement(eng, out):
    for which in ("connect_cross", "connect_final"):
        gs = ragged_sets(*eng.lists(which))
        bad = [v for v in range(len(gs)) if gs[v] != frozenset(out[which][v])]
        assert not bad, f"{which}: {len(bad)} of {len(gs)} voxels differ, first {bad[:5]}: gpu={sorted(gs[bad[0]])} restated={sorted(out[which][bad[0]])}"
    root, kept = eng.node_labels()
    np.testing.assert_array_equal(root, out["root"])
    np.testing.assert_array_equal(kept, out["kept"])
    np.testing.assert_array_equal(eng.point_labels(), out["point_labels"])
    c = eng.counts()
    assert {k: c[k] for k in ("clusters", "kept", "isolated", "reattached")} == out["counts"]


def test_truth_by_construction(case):
    sc, eng = case["sc"], case["eng"]
    t = _check_truth(sc, eng, case["truth"])
    if "size" in sc:         # cliques, rods, single cells and pairs: the component is the clique or the rod
        np.testing.assert_array_equal(t["size"][t["vox"]], sc["size"])
        np.testing.assert_array_equal(t["kept"][t["vox"]] >= 0, sc["size"] > sc["params"]["voxels_min"])
    if sc.get("clique"):     # ... and so is every row and every list
        for w in ("adjacency", "connect_cut", "connect_cross", "connect_final"):
            np.testing.assert_array_equal(np.diff(eng.lists(w)[0])[t["vox"]], sc["size"], err_msg=w)
    if "last_cell" in sc:    # the voxel whose keep_rank + keep_flag is the number of kept segments
        assert t["vox"][sc["last_cell"]] == eng.counts()["voxels"] - 1


def test_restatement_over_the_engines_own_rows(case, oracle):
    _check_restatement(case["eng"], _restate(oracle, case["eng"], case["p"]))


def test_oracle_end_to_end(case):
    eng, ref = case["eng"], case["ref"]
    for which in ("connect_cross", "connect_final"):
        gs, rs = ragged_sets(*eng.lists(which)), ragged_sets(*ref.lists(which))
        bad = [v for v in range(len(rs)) if gs[v] != rs[v]]
        assert not bad, f"{which}: {len(bad)} of {len(rs)} voxels differ, first {bad[:5]}: gpu={sorted(gs[bad[0]])} ref={sorted(rs[bad[0]])}"
    pl_ref, nc_ref = ref.labels()
    root, _ = eng.node_labels()
    np.testing.assert_array_equal(canonical_labels(root), canonical_labels(nc_ref))
    np.testing.assert_array_equal(eng.point_labels(), pl_ref)
    cand, succ, _ = _oracle_closest_check(ref, case["p"].adjacency_min)
    c = eng.counts()
    assert (c["clusters"], c["kept"], c["isolated"], c["reattached"]) == (ref.clusters_num, ref.kept_clusters, len(cand), len(succ))


def test_full_clique_ladder(gpu, oracle):
    """All eighteen clique sizes, rows of 1 .. 513 entries: the truth by construction and the restatement (the oracle leg is ladder_oracle's)."""
    sc = ms.clique_ladder()
    p = gpu.default_params(2, **sc["params"])
    eng = _engine(gpu, p, sc["xyz"], None)
    t = _check_truth(sc, eng)
    lens = {w: np.diff(eng.lists(w)[0])[t["vox"]] for w in ("adjacency", "connect_cut", "connect_cross", "connect_final")}
    for w, n in lens.items():
        np.testing.assert_array_equal(n, sc["size"], err_msg=w)
    print("clique ladder: row lengths", sorted(set(lens["connect_final"].tolist())), "schedule", eng.schedule_counters())
    assert set(lens["connect_final"].tolist()) == set(ms.LADDER)
    _check_restatement(eng, _restate(oracle, eng, p))
    eng.run()
    _check_truth(sc, eng)


def _arrays(eng):
    out = [eng.point_labels().copy()] + [a.copy() for a in eng.node_labels()]
    for which in ("connect_cross", "connect_final"):
        off, idx = eng.lists(which)
        out += [off.copy(), idx.copy()]
    c = eng.counts()
    return out + [np.array([c[k] for k in ("voxels", "used", "clusters", "kept", "isolated", "reattached")])]


REPEAT = [("snake", ms.snake), ("rods_vm3", lambda: ms.rods(voxels_min=3)), ("chains", ms.chains)]


@pytest.mark.parametrize("knob", ROUTES, ids=["fork", "no_overlap"])
@pytest.mark.parametrize("name,build", REPEAT, ids=[r[0] for r in REPEAT])
def test_more_runs_and_a_fresh_engine_repeat_every_array(gpu, name, build, knob):
    """Unions, path halving and k_flatten run while other workgroups write `parent`: a race would show as an array that moves.  Every
    result is compared with the truth, not only with the first run."""
    sc = _scene(name, build)
    p = gpu.default_params(2, **sc["params"])
    eng = _engine(gpu, p, sc["xyz"], knob)
    first = _arrays(eng)
    _check_truth(sc, eng)
    for _ in range(3):
        eng.run()
        _check_truth(sc, eng)
        for a, b in zip(first, _arrays(eng)):
            np.testing.assert_array_equal(a, b)
    e2 = _engine(gpu, p, sc["xyz"], knob)
    _check_truth(sc, e2)
    for a, b in zip(first, _arrays(e2)):
        np.testing.assert_array_equal(a, b)
