"""The C++ mirror of absorbing small label parts (include/vgs_segmentation.hpp: absorbLabelParts on both classes) through
vgs_run --refine --absorbed-labels, against Engine.absorb_label_parts for the same task: the written labels byte for byte and the eight
counts of the stdout line; the --refined-* tables beside it keep describing the refined labels."""
import subprocess

import numpy as np
import pytest

from test_cpp_segment_desc import CSRC, RUN, SVGS_LINES, VGS_LINES, _write_task


@pytest.mark.gpu
@pytest.mark.parametrize("method", [2, 3], ids=["vgs", "svgs"])
def test_absorbed_labels_match_the_engine(gpu, tmp_path, method):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    xyz = gpu.scenes.town_scene(60_000)
    gpu.pcd.write_pcd(tmp_path / "in.pcd", xyz, mode="binary")
    lines = dict(VGS_LINES if method == 2 else SVGS_LINES)
    lines.update({12: str(tmp_path) + "/", 15: "in.pcd", 18: str(tmp_path) + "/", 21: "out.pcd"})
    task = str(tmp_path / "task.txt")
    _write_task(task, method, lines)
    f = {n: tmp_path / n for n in ("a.i32", "parts.csv", "parts_alone.csv", "ids.i32", "ids_alone.i32")}
    kw = dict(min_points=200, island_points=5000, max_rounds=3, drop=True)
    flags = ["--absorb-min-points", "200", "--absorb-islands", "5000", "--absorb-rounds", "3", "--absorb-drop"]
    parts = ["--refine", "--refined-components"]
    out = subprocess.run([RUN, task] + parts + [str(f["parts.csv"]), "--component-ids", str(f["ids.i32"]), "--absorbed-labels", str(f["a.i32"])] + flags,
                         check=True, capture_output=True, text=True).stdout
    eng = gpu.Engine(gpu.default_params(method))
    eng.set_points(xyz)
    eng.run()
    eng.refine_labels()
    want = eng.absorb_label_parts(eng.refined_labels(), K=eng.counts()["kept"], **kw)
    assert want["parts_absorbed"] > 0 and want["rounds"] >= 1
    got = np.fromfile(f["a.i32"], dtype=np.int32)
    assert got.tobytes() == want["labels"].tobytes()
    line = [l for l in out.splitlines() if l.startswith("absorbed ")]
    assert len(line) == 1 and [int(v) for v in line[0].split()[1:]] == [want[k] for k in gpu.Engine.ABSORB_COUNTS]
    # the call changes no other output: the parts of the refined labels are what a run without it writes
    subprocess.check_call([RUN, task] + parts + [str(f["parts_alone.csv"]), "--component-ids", str(f["ids_alone.i32"])], stdout=subprocess.DEVNULL)
    assert f["parts.csv"].read_bytes() == f["parts_alone.csv"].read_bytes() and f["ids.i32"].read_bytes() == f["ids_alone.i32"].read_bytes()
    assert got.tobytes() != eng.refined_labels().tobytes()
