"""vgs_run --segment-boxes: the oriented-box CSV of the task-file front end (examples/drivers.hpp -> getClusterBoxes of
include/vgs_segmentation.hpp) against Engine.segment_boxes() for the same task and both --box-frame values; the --segments file of the
same invocation against one written without the new flag; and the class-level getter before segmentation."""
import subprocess

import numpy as np
import pytest

from test_cpp_segment_desc import CSRC, RUN, SVGS_LINES, VGS_LINES, _write_task


def _run(gpu, tmp_path, method, xyz, frame):
    gpu.pcd.write_pcd(tmp_path / "in.pcd", xyz, mode="binary")
    lines = dict(VGS_LINES if method == 2 else SVGS_LINES)
    lines.update({12: str(tmp_path) + "/", 15: "in.pcd", 18: str(tmp_path) + "/", 21: "out.pcd"})
    _write_task(tmp_path / "task.txt", method, lines)
    plain, seg, box = tmp_path / "plain.csv", tmp_path / f"segments_{frame}.csv", tmp_path / f"boxes_{frame}.csv"
    if not plain.exists():
        subprocess.check_call([RUN, str(tmp_path / "task.txt"), "--segments", str(plain)], stdout=subprocess.DEVNULL)
    args = [RUN, str(tmp_path / "task.txt"), "--segments", str(seg), "--segment-boxes", str(box)]
    subprocess.check_call(args + (["--box-frame", frame] if frame != "default" else []), stdout=subprocess.DEVNULL)
    assert seg.read_bytes() == plain.read_bytes()   # the --segments file does not depend on the new flag
    with open(box) as f:
        header = f.readline().strip().split(",")
    rows = np.loadtxt(box, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    assert len(header) == 22 and header[0] == "label" and rows.shape[1] == 22
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("method", [2, 3], ids=["vgs", "svgs"])
def test_boxes_csv_matches_engine(gpu, tmp_path, method):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    xyz = gpu.scenes.town_scene(60_000)
    eng = gpu.Engine(gpu.default_params(method))
    eng.set_points(xyz)
    eng.run()
    for flag, frame in (("default", "principal"), ("principal", "principal"), ("upright", "upright")):
        rows = _run(gpu, tmp_path, method, xyz, flag)
        b = eng.segment_boxes(frame)
        K = b["lo3"].shape[0]
        assert K > 0 and rows.shape[0] == K
        assert np.array_equal(rows[:, 0], np.arange(K))
        # %.17g doubles read back exactly
        got = dict(center3=rows[:, 1:4], half3=rows[:, 4:7], frame9=rows[:, 7:16], lo3=rows[:, 16:19], hi3=rows[:, 19:22])
        for k in b:
            assert np.array_equal(got[k], b[k]), (flag, k)


def test_bad_box_frame_is_a_usage_error(tmp_path):
    """Argument parsing only: no device needed."""
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    r = subprocess.run([RUN, str(tmp_path / "none.txt"), "--segment-boxes", str(tmp_path / "b.csv"), "--box-frame", "tilted"], capture_output=True)
    assert r.returncode == 2 and b"principal or upright" in r.stderr


@pytest.mark.gpu
def test_get_cluster_boxes_before_segmentation(gpu):
    """The classes: SuperVoxelBasedSegmentation raises the state error until the cloud is segmented, VoxelBasedSegmentation returns
    nothing before drawColorMapofPointsinClusters, as getClusterDescriptors does."""
    xyz = gpu.scenes.town_scene(60_000)
    s = gpu.SuperVoxelBasedSegmentation(0.05)
    s.setInputCloud(xyz); s.getCloudPointNum(xyz); s.addPointsFromInputCloud()
    for frame in ("principal", "upright"):
        with pytest.raises(gpu.VgsError) as e:
            s.getClusterBoxes(frame)
        assert e.value.status == gpu._lib.VGS_E_STATE
    v = gpu.VoxelBasedSegmentation(0.15)
    v.setInputCloud(xyz); v.getCloudPointNum(xyz); v.addPointsFromInputCloud()
    assert all(a.shape[0] == 0 for a in v.getClusterBoxes().values())
