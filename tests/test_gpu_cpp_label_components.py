"""The C++ mirror of the connected parts of a labelling (include/vgs_segmentation.hpp: getLabelComponents on both classes) through
vgs_run --refine --refined-components / --class-components / --component-ids, against Engine.label_components for the same task, by
value: the CSV of --refined-components round-trips to the Python table, and so do the raw part ids."""
import subprocess

import numpy as np
import pytest

from test_cpp_segment_desc import CSRC, RUN, SVGS_LINES, VGS_LINES, _write_task


def _table(got):
    C = got["n_parts"]
    largest = np.zeros(C, np.int64)
    largest[got["label_largest"][got["label_largest"] >= 0]] = 1
    return np.stack([np.arange(C), got["part_label"], got["part_points"], got["part_nodes"], got["part_first_node"], largest], axis=1).astype(np.int64)


def _rows(path):
    rows = np.loadtxt(path, delimiter=",", skiprows=1, dtype=np.int64, ndmin=2)
    return rows.reshape(-1, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("method", [2, 3], ids=["vgs", "svgs"])
def test_component_csvs_match_the_engine(gpu, tmp_path, method):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    xyz = gpu.scenes.town_scene(60_000)
    cell = np.floor(xyz[:, :2].astype(np.float64)).astype(np.int64)
    cls = ((cell[:, 0] + 2 * cell[:, 1]) % 6 - 1).astype(np.int32)   # classes -1 .. 4 in 1 m cells of the ground plan
    assert np.array_equal(np.unique(cls), np.arange(-1, 5))
    gpu.pcd.write_pcd(tmp_path / "in.pcd", xyz, mode="binary", extra={"cls": cls})
    lines = dict(VGS_LINES if method == 2 else SVGS_LINES)
    lines.update({12: str(tmp_path) + "/", 15: "in.pcd", 18: str(tmp_path) + "/", 21: "out.pcd"})
    task = str(tmp_path / "task.txt")
    _write_task(task, method, lines)
    f = {n: tmp_path / n for n in ("r.csv", "r.i32", "c.csv", "c.i32", "both_r.csv", "both_c.csv")}
    subprocess.check_call([RUN, task, "--refine", "--refined-components", str(f["r.csv"]), "--component-ids", str(f["r.i32"])], stdout=subprocess.DEVNULL)
    subprocess.check_call([RUN, task, "--class-components", str(f["c.csv"]), "--class-field", "cls", "--classes", "5", "--component-ids", str(f["c.i32"])],
                          stdout=subprocess.DEVNULL)
    subprocess.check_call([RUN, task, "--refine", "--refined-components", str(f["both_r.csv"]), "--class-components", str(f["both_c.csv"]),
                           "--class-field", "cls", "--classes", "5"], stdout=subprocess.DEVNULL)
    assert f["both_r.csv"].read_bytes() == f["r.csv"].read_bytes() and f["both_c.csv"].read_bytes() == f["c.csv"].read_bytes()
    eng = gpu.Engine(gpu.default_params(method))
    eng.set_points(xyz)
    eng.run()
    eng.refine_labels()
    refined, K = eng.refined_labels(), eng.counts()["kept"]
    got = eng.label_components(refined, K)
    assert got["n_parts"] >= K > 0
    assert np.array_equal(_rows(f["r.csv"]), _table(got))
    assert np.array_equal(np.fromfile(f["r.i32"], dtype=np.int32), got["part_of_point"])
    got = eng.label_components(cls, 5)
    assert got["n_parts"] >= 5 and (np.diff(got["label_first"]) >= 1).all()
    assert np.array_equal(_rows(f["c.csv"]), _table(got))
    assert np.array_equal(np.fromfile(f["c.i32"], dtype=np.int32), got["part_of_point"])
    # a class the field holds but --classes does not cover ends the run with the library's message
    r = subprocess.run([RUN, task, "--class-components", str(tmp_path / "x.csv"), "--class-field", "cls", "--classes", "3"], capture_output=True)
    assert r.returncode == 1 and b"is not below K = 3" in r.stderr
