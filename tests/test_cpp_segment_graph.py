"""vgs_run --segment-graph / --segment-adjacency: the cluster adjacency graph of the task-file front end (examples/drivers.hpp ->
getClusterGraph / getClusterAdjacency of include/vgs_segmentation.hpp) against Engine.segment_graph() for the same task, and the multimap
of getClusterAdjacency (PCL's getSupervoxelAdjacency idiom) against the CSV."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_segment_desc import SVGS_LINES, VGS_LINES, _write_task

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
RUN = os.path.join(ROOT, "examples", "vgs_run")


def _run_graph(gpu, tmp_path, method, xyz):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    gpu.pcd.write_pcd(tmp_path / "in.pcd", xyz, mode="binary")
    lines = dict(VGS_LINES if method == 2 else SVGS_LINES)
    lines.update({12: str(tmp_path) + "/", 15: "in.pcd", 18: str(tmp_path) + "/", 21: "out.pcd"})
    _write_task(tmp_path / "task.txt", method, lines)
    csv, adj = tmp_path / "graph.csv", tmp_path / "adjacency.txt"
    subprocess.check_call([RUN, str(tmp_path / "task.txt"), "--segment-graph", str(csv), "--segment-adjacency", str(adj)], stdout=subprocess.DEVNULL)
    with open(csv) as f:
        header = f.readline().strip().split(",")
    assert header == ["a", "b", "n_pairs", "n_finite", "nodes_a", "nodes_b", "w_mean", "w_min", "w_max"]
    rows = np.loadtxt(csv, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    pairs = np.loadtxt(adj, delimiter=",", dtype=np.int64, ndmin=2)
    return rows, pairs


@pytest.mark.gpu
@pytest.mark.parametrize("method", [2, 3], ids=["vgs", "svgs"])
def test_segment_graph_csv_matches_engine(gpu, tmp_path, method):
    xyz = gpu.scenes.town_scene(60_000)
    rows, pairs = _run_graph(gpu, tmp_path, method, xyz)
    eng = gpu.Engine(gpu.default_params(method))
    eng.set_points(xyz)
    eng.run()
    g = eng.segment_graph()
    E = g["seg_ab"].shape[0]
    assert E > 0 and rows.shape == (E, 9)
    assert np.array_equal(rows[:, 0:2].astype(np.int32), g["seg_ab"])
    assert np.array_equal(rows[:, 2].astype(np.int64), g["n_pairs"])
    assert np.array_equal(rows[:, 3].astype(np.int64), g["n_finite"])
    assert np.array_equal(rows[:, 4:6].astype(np.int32), g["nodes_ab"])
    # %.17g doubles and %.9g floats read back exactly
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(g["n_finite"] > 0, g["w_sum"] / g["n_finite"], np.nan)
    assert np.array_equal(rows[:, 6], mean, equal_nan=True)
    assert np.array_equal(rows[:, 7].astype(np.float32), g["w_min"], equal_nan=True)
    assert np.array_equal(rows[:, 8].astype(np.float32), g["w_max"], equal_nan=True)
    # getClusterAdjacency: both directions of every edge, in multimap order (key ascending, equal keys in insertion order)
    ab = g["seg_ab"].astype(np.int64)
    both = np.concatenate([ab, ab[:, ::-1]])
    want = both[np.lexsort((both[:, 1], both[:, 0]))]
    assert pairs.shape == (2 * E, 2)
    assert np.array_equal(pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))], want)
    assert (np.diff(pairs[:, 0]) >= 0).all()
