"""The C++ mirror of the adjacency graph of a labelling (include/vgs_segmentation.hpp: getLabelGraph on both classes) through
vgs_run --refine --refined-graph / --class-graph, against Engine.label_graph for the same task, value for value: the CSV round-trips to
the Python table (w_mean is w_sum / n_finite in fp64 on both sides)."""
import subprocess

import numpy as np
import pytest

from test_cpp_segment_desc import CSRC, RUN, SVGS_LINES, VGS_LINES, _write_task

COLUMNS = "a,b,n_shared,n_pairs,n_finite,nodes_a,nodes_b,w_mean,w_min,w_max"


def _table(got):
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(got["n_finite"] > 0, got["w_sum"] / got["n_finite"].astype(np.float64), np.nan)
    ints = np.concatenate([got["seg_ab"], got["n_shared"][:, None], got["n_pairs"][:, None], got["n_finite"][:, None], got["nodes_ab"]], axis=1)
    return ints.astype(np.int64), mean, got["w_min"], got["w_max"]


def _same(path, got):
    with open(path) as f:
        assert f.readline().strip() == COLUMNS
    rows = np.loadtxt(path, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2).reshape(-1, 10)
    ints, mean, mn, mx = _table(got)
    assert rows.shape[0] == got["n_edges"]
    assert np.array_equal(rows[:, :7].astype(np.int64), ints)
    assert rows[:, 7].tobytes() == mean.tobytes()
    assert rows[:, 8].astype(np.float32).tobytes() == mn.tobytes() and rows[:, 9].astype(np.float32).tobytes() == mx.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("method", [2, 3], ids=["vgs", "svgs"])
def test_graph_csvs_match_the_engine(gpu, tmp_path, method):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    xyz = gpu.scenes.town_scene(60_000)
    cell = np.floor(xyz[:, :2].astype(np.float64)).astype(np.int64)
    cls = ((cell[:, 0] + 2 * cell[:, 1]) % 6 - 1).astype(np.int32)   # classes -1 .. 4 in 1 m cells of the ground plan
    gpu.pcd.write_pcd(tmp_path / "in.pcd", xyz, mode="binary", extra={"cls": cls})
    lines = dict(VGS_LINES if method == 2 else SVGS_LINES)
    lines.update({12: str(tmp_path) + "/", 15: "in.pcd", 18: str(tmp_path) + "/", 21: "out.pcd"})
    task = str(tmp_path / "task.txt")
    _write_task(task, method, lines)
    f = {n: tmp_path / n for n in ("r.csv", "c.csv", "parts.csv")}
    subprocess.check_call([RUN, task, "--refine", "--refined-graph", str(f["r.csv"]), "--class-graph", str(f["c.csv"]), "--class-components",
                           str(f["parts.csv"]), "--class-field", "cls", "--classes", "5"], stdout=subprocess.DEVNULL)
    eng = gpu.Engine(gpu.default_params(method))
    eng.set_points(xyz)
    eng.run()
    eng.refine_labels()
    got = eng.label_graph(eng.refined_labels(), eng.counts()["kept"])
    assert got["n_edges"] > 0 and got["n_finite"].sum() > 0
    _same(f["r.csv"], got)
    got = eng.label_graph(cls, 5)
    assert got["n_edges"] >= 5 and (got["n_shared"] > 0).any()
    _same(f["c.csv"], got)
    assert f["parts.csv"].stat().st_size > 0   # the parts of the same field beside it
    # the usage rules of the companions
    r = subprocess.run([RUN, task, "--refined-graph", str(tmp_path / "x.csv")], capture_output=True)
    assert r.returncode == 2 and b"--refined-graph needs --refine" in r.stderr
    r = subprocess.run([RUN, task, "--class-graph", str(tmp_path / "x.csv"), "--classes", "5"], capture_output=True)
    assert r.returncode == 2 and b"--class-graph needs --class-field" in r.stderr
    r = subprocess.run([RUN, task, "--class-graph", str(tmp_path / "x.csv"), "--class-field", "cls", "--classes", "3"], capture_output=True)
    assert r.returncode == 1 and b"is not below K = 3" in r.stderr
