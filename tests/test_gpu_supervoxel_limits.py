"""The supervoxel stage (csrc/vccs.hip, 28 kernels) and the SVGS node graph (csrc/svgs.hip) on the paths that street-like scenes do not
reach, against the CPU oracle, every comparison exact:
  * svgs_supervoxels in both vccs_modes on the scenes of tests/supervoxel_scenes.py -- more labels in a tile than the LDS table has slots,
    more labels among 256 voxels than k_vccs_reseed's table holds, six and more supervoxels in one 27-neighbourhood, tiles staged and not
    staged by k_pclt_normals, tiles of more than 64 voxels with shells of more than 128, voxels 32 m and more from their tile's first
    voxel, no expansion round at all, every seed rejected, a chain of 1 200 supervoxels, clouds of one and two points -- label for label,
    then end to end through run();
  * svgs_segment on a caller's labels: one neighbour row of 64, 65, 128, 129 and 512 entries (every size of k_sv_neighbours' sorting
    network), the reported overflow at 513, ties on d2, the strict d2 < r2 one float step to either side, sparse / negative / too large
    labels, max_label <= 1, all-zero labels, and non-finite points that carry a supervoxel's label.
tests/test_supervoxel_scenes_cpu.py proves on the oracle alone that every scene reaches the path it is named for."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import supervoxel_scenes as S
from helpers import canonical_labels, oracle_params, ragged_lists, ragged_sets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (0, 1)


def _params(gpu, kw, mode):
    return gpu.default_params(3, vccs_mode=mode, **kw)


_REF = {}


def _reference(oracle, gpu, name, mode):
    """The oracle's supervoxels of a scene, once per module: (xyz, kw, labels, max_label, seeds)."""
    if (name, mode) not in _REF:
        xyz, kw = S.SUPERVOXEL_SCENES[name]()
        p = oracle_params(oracle, _params(gpu, kw, mode))
        if mode == 0:
            lab, mx = oracle.vccs(xyz, p)
            seeds = mx
        else:
            lab, mx, seeds = oracle.vccs_pcl_seeds(xyz, p)
        _REF[(name, mode)] = (xyz, kw, lab, mx, seeds)
    return _REF[(name, mode)]


def _supervoxels(gpu, xyz, kw, mode):
    eng = gpu.Engine(_params(gpu, kw, mode))
    eng.set_points(xyz)
    eng.supervoxels()
    return eng


# ---------------------------------------------------------------- svgs_supervoxels
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(S.SUPERVOXEL_SCENES))
def test_supervoxel_labels_match_the_oracle(gpu, oracle, name, mode):
    """After svgs_supervoxels alone: the labels and max_label of the oracle's restatement point for point (oracle.vccs / oracle.vccs_pcl),
    the same supervoxel count (vccs_mode 1: the seeds that survive the rejection), one label per voxel, and the same bytes from a second
    call and from a fresh engine."""
    xyz, kw, ref_lab, ref_mx, ref_seeds = _reference(oracle, gpu, name, mode)
    eng = _supervoxels(gpu, xyz, kw, mode)
    lab, mx = eng.supervoxel_labels()
    print(f"SUPERVOXELS {name} m{mode}: max_label={mx} (oracle {ref_mx}), supervoxels={eng.counts()['supervoxels']} (oracle {ref_seeds}), "
          f"differing points={int((lab != ref_lab).sum())} of {lab.size}")
    assert mx == ref_mx
    np.testing.assert_array_equal(lab, ref_lab)
    assert eng.counts()["supervoxels"] == ref_seeds
    T = oracle.voxelize(xyz, kw["voxel_size"], bbox_first=bool(mode)).voxel_table()
    S.voxel_labels(T, lab)   # asserts: all points of a voxel share one label
    eng.supervoxels()
    lab2, mx2 = eng.supervoxel_labels()
    assert mx2 == mx and lab2.tobytes() == lab.tobytes()
    lab3, mx3 = _supervoxels(gpu, xyz, kw, mode).supervoxel_labels()
    assert mx3 == mx and lab3.tobytes() == lab.tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", S.END_TO_END)
def test_end_to_end(gpu, oracle, name, mode):
    """run() = svgs_supervoxels + svgs_segment against the oracle's pipeline on the engine's own labels: point labels and cluster count.
    all_rejected in vccs_mode 1 and the clouds of one voxel reach svgs_segment without a single supervoxel."""
    xyz, kw, ref_lab, ref_mx, _ = _reference(oracle, gpu, name, mode)
    p = _params(gpu, kw, mode)
    eng = gpu.Engine(p)
    eng.set_points(xyz)
    eng.run()
    lab, mx = eng.supervoxel_labels()
    assert mx == ref_mx
    np.testing.assert_array_equal(lab, ref_lab)
    ref = oracle.run_svgs_from_labels(xyz, lab, mx, oracle_params(oracle, p))
    c = eng.counts()
    print(f"END TO END {name} m{mode}: supervoxels={c['voxels']} (oracle {ref.V}), clusters={c['clusters']} (oracle {ref.clusters_num})")
    assert c["voxels"] == ref.V
    np.testing.assert_array_equal(eng.point_labels(), ref.labels()[0])
    assert c["clusters"] == ref.clusters_num and c["kept"] == ref.kept_clusters


@pytest.mark.parametrize("mode", MODES)
def test_seed_size_must_exceed_voxel_size(gpu, oracle, mode):
    """seed_size == voxel_size and seed_size < voxel_size are refused; the engine then runs a valid parameter set to the oracle's labels."""
    from vgs_svgs_segmentation_amd._lib import VgsError
    xyz, kw, ref_lab, ref_mx, _ = _reference(oracle, gpu, "block_2p5_origin", mode)
    eng = gpu.Engine(_params(gpu, dict(kw, seed_size=kw["voxel_size"]), mode))
    eng.set_points(xyz)
    with pytest.raises(VgsError):
        eng.supervoxels()
    eng.set_params(_params(gpu, dict(kw, seed_size=0.5 * kw["voxel_size"]), mode))
    with pytest.raises(VgsError):
        eng.supervoxels()
    with pytest.raises(VgsError):
        eng.run()
    with pytest.raises(VgsError):
        eng.supervoxel_labels()
    eng.set_params(_params(gpu, kw, mode))
    eng.supervoxels()
    lab, mx = eng.supervoxel_labels()
    assert mx == ref_mx
    np.testing.assert_array_equal(lab, ref_lab)


_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
import vgs_svgs_segmentation_amd as v
from supervoxel_scenes import line_3000
xyz, kw = line_3000()
eng = v.Engine(v.default_params(3, vccs_mode=1, **kw))
eng.set_points(xyz)
eng.supervoxels()
lab, mx = eng.supervoxel_labels()
np.save(sys.argv[2], np.append(lab, mx))
"""


def test_sweep_chain_of_the_line(gpu, oracle, tmp_path):
    """line_3000 in vccs_mode 1, once in a fresh child process with VGS_DEBUG set: the driver prints how many rounds met their first
    unchanged sweep at which index.  The first batch of a round is four sweeps (indices 0 .. 3); an index above 3 would mean that a later
    batch ran.  Observed on an MI355X: {1: 7, 2: 11} -- seven of the eighteen rounds settled at sweep 1 and eleven at sweep 2, the largest
    index is 2.  The chain of 1 200 supervoxels does NOT take the driver beyond the first batch (a supervoxel of a line takes voxels from
    its two neighbours only, so the live flags settle in two or three sweeps whatever the length of the chain); the scene was not tuned
    against that output, and what is asserted is the equality with the oracle and that every round reported its fixed point."""
    xyz, kw, ref_lab, ref_mx, _ = _reference(oracle, gpu, "line_3000", 1)
    out = tmp_path / "labels.npy"
    env = dict(os.environ, VGS_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(out)
    assert got[-1] == ref_mx
    np.testing.assert_array_equal(got[:-1], ref_lab)
    line = [ln for ln in r.stderr.splitlines() if "rounds by the index of their first unchanged sweep" in ln]
    assert len(line) == 1, r.stderr[-3000:]
    hist = {int(a): int(b) for a, b in re.findall(r"(\d+):(\d+)", line[0].split("sweep:")[1])}
    print(f"SWEEPS line_3000: {hist}")
    rounds = 6 * (int(np.float32(1.8) * np.float32(kw["seed_size"]) / np.float32(kw["voxel_size"])) - 1)
    assert sum(hist.values()) == rounds   # six passes of depth - 1 rounds, each settled once


# ---------------------------------------------------------------- svgs_segment on a caller's labels
_SEG = {}


def _segment_reference(oracle, gpu, key, build):
    if key not in _SEG:
        scene = build()
        ref = oracle.run_svgs_from_labels(scene[0], scene[1], scene[2], oracle_params(oracle, gpu.default_params(3)))
        _SEG[key] = (scene, ref)
    return _SEG[key]


def _segment(gpu, xyz, labels, max_label, eng=None):
    eng = eng or gpu.Engine(gpu.default_params(3))
    eng.set_points(xyz)
    eng.set_supervoxel_labels(labels, max_label)
    eng.svgs_segment()
    return eng


def _check_segmentation(eng, ref):
    """Adjacency rows in exact order, the three connect lists as sets and element for element in "reference" order, node labels, point
    labels and counts: all equal to the oracle's."""
    c = eng.counts()
    assert c["voxels"] == c["supervoxels"] == ref.V
    go, gi = eng.lists("adjacency")
    ro, ri = ref.lists("adjacency")
    assert ragged_lists(go, gi) == ragged_lists(ro, ri)
    assert c["adj"] == ref.E
    for which in ("connect_cut", "connect_cross", "connect_final"):
        ro, ri = ref.lists(which)
        assert ragged_sets(*eng.lists(which)) == ragged_sets(ro, ri), which
        go, gi = eng.lists(which, "reference")
        np.testing.assert_array_equal(go, ro)
        np.testing.assert_array_equal(gi, ri)
    pl, nc = ref.labels()
    root, _ = eng.node_labels()
    np.testing.assert_array_equal(canonical_labels(root), canonical_labels(nc))
    np.testing.assert_array_equal(eng.point_labels(), pl)
    assert c["clusters"] == ref.clusters_num and c["kept"] == ref.kept_clusters
    return go, gi


@pytest.mark.parametrize("size", S.HUB_SIZES)
def test_hub_row(gpu, oracle, size):
    """The hub's row holds all S supervoxels: 64 and 65 (the 64- and the 128-entry network), 128 and 129 (128 without padding, 256), 512
    (the last row that fits: it holds the hub itself because d2 = 0 < r2)."""
    (xyz, lab, mx), ref = _segment_reference(oracle, gpu, size, lambda: S.hub_and_shell(size))
    eng = _segment(gpu, xyz, lab, mx)
    _check_segmentation(eng, ref)
    rows = eng.adjacency_counts()
    assert rows.max() == rows[0] == size


def test_row_overflow_is_reported(gpu, oracle):
    """513 entries: svgs_segment raises an error that names the limit; the same engine then runs the 512-entry scene correctly."""
    from vgs_svgs_segmentation_amd._lib import VgsError
    xyz, lab, mx = S.hub_and_shell(S.SV_ROW + 1)
    eng = gpu.Engine(gpu.default_params(3))
    eng.set_points(xyz)
    eng.set_supervoxel_labels(lab, mx)
    with pytest.raises(VgsError, match=str(S.SV_ROW)):
        eng.svgs_segment()
    (xyz, lab, mx), ref = _segment_reference(oracle, gpu, S.SV_ROW, lambda: S.hub_and_shell(S.SV_ROW))
    _check_segmentation(_segment(gpu, xyz, lab, mx, eng), ref)


def test_hub_edges(gpu, oracle):
    """A negative centre, two supervoxels with one centroid (a tie on d2, broken by id), and centroids one float step inside, on and one step
    outside graph_size: d2 < r2 is strict."""
    (xyz, lab, mx, ids), ref = _segment_reference(oracle, gpu, "edges", S.hub_edges)
    eng = _segment(gpu, xyz, lab, mx)
    _check_segmentation(eng, ref)
    off, idx = eng.lists("adjacency")
    row = idx[off[0]:off[1]].tolist()
    assert len(row) == 129 and row[0] == ids["hub"] and row[-1] == ids["inside"]
    assert ids["on"] not in row and ids["outside"] not in row
    a, b = ids["twins"]
    assert row.index(b) == row.index(a) + 1
    cen = eng.attributes()["centroid"]
    assert np.array_equal(cen[a].view(np.uint32), cen[b].view(np.uint32))
    assert np.array_equal(cen[ids["hub"]], np.array(S.EDGE_HUB, dtype=np.float32))


@pytest.mark.parametrize("name", list(S.labellings_40()))
def test_labellings(gpu, oracle, name):
    """Sparse ids, negative labels, labels of max_label and above, max_label <= 1 and all-zero labels: the supervoxel table, the counts and
    the point labels of the oracle; without a supervoxel, empty descriptor and graph tables instead of an error."""
    (xyz, lab, mx, V, unlabelled), ref = _segment_reference(oracle, gpu, name, lambda: S.labellings_40()[name])
    eng = _segment(gpu, xyz, lab, mx)
    c = eng.counts()
    assert c["voxels"] == c["supervoxels"] == ref.V == V
    off, idx = ref.lists("sv_points")
    t = eng.voxel_table()
    np.testing.assert_array_equal(t["start"], off.astype(np.int32))
    np.testing.assert_array_equal(t["point_idx"], idx)
    assert c["finite"] == idx.shape[0] == xyz.shape[0] - unlabelled
    assert c["clusters"] == ref.clusters_num and c["kept"] == ref.kept_clusters
    pl = eng.point_labels()
    np.testing.assert_array_equal(pl, ref.labels()[0])
    assert int((pl < 0).sum()) == unlabelled
    if V == 0:
        assert c["clusters"] == c["kept"] == 0 and (pl == -1).all()
        d, g = eng.segment_descriptors(), eng.segment_graph()
        assert all(v.shape[0] == 0 for v in d.values()) and all(v.shape[0] == 0 for v in g.values())
    else:
        _check_segmentation(eng, ref)


def test_non_finite_points_belong_to_no_supervoxel(gpu, oracle):
    """include/vgs.h: a point with a non-finite coordinate belongs to no supervoxel, whatever label the caller gave it (k_sv_keys gives it
    the invalid key).  The engine on the NaN labelling equals the engine on the same cloud with those points labelled 0, and the oracle;
    every centroid is finite."""
    xyz, lab, mx, bad = S.nan_labelling()
    ref = oracle.run_svgs_from_labels(xyz, lab, mx, oracle_params(oracle, gpu.default_params(3)))
    a = _segment(gpu, xyz, lab, mx)
    b = _segment(gpu, xyz, np.where(bad, 0, lab).astype(np.int32), mx)
    _check_segmentation(a, ref)
    assert np.isfinite(a.attributes()["centroid"]).all()
    pl = a.point_labels()
    assert (pl[bad] == -1).all() and (pl[~bad] >= 0).all()
    np.testing.assert_array_equal(pl, b.point_labels())
    ta, tb = a.voxel_table(), b.voxel_table()
    for k in ("start", "point_idx"):
        np.testing.assert_array_equal(ta[k], tb[k])
    assert a.counts()["finite"] == xyz.shape[0] - int(bad.sum())
    ga, gb = a.attributes(), b.attributes()
    for k in ga:
        assert np.array_equal(ga[k].view(np.uint8), gb[k].view(np.uint8)), k
    off, idx = ref.lists("sv_points")
    np.testing.assert_array_equal(ta["point_idx"], idx)
