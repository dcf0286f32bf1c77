"""vgs_run --refine: the coloured PCD of the task-file front end written from the point-level refined labels (examples/drivers.hpp ->
refineClusterLabels of include/vgs_segmentation.hpp) against Engine.refined_labels() for the same task: clusters in label order, points in
ascending index, so the file's points are the header's labels regrouped; with the default parameters and with --patch-radius,
--switch-ratio and --no-fill; and the usage errors of the new flags."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_segment_desc import CSRC, RUN, SVGS_LINES, VGS_LINES, _write_task
from test_segdesc_resources import HIPCC


def _grouping(labels):
    K = int(labels.max()) + 1
    order = np.argsort(labels, kind="stable")   # label order, ascending index inside a label
    order = order[labels[order] >= 0]
    return order, np.concatenate([[0], np.cumsum(np.bincount(labels[labels >= 0], minlength=K))])


@pytest.mark.gpu
@pytest.mark.parametrize("method", [2, 3], ids=["vgs", "svgs"])
def test_refined_pcd_matches_engine(gpu, tmp_path, method):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    xyz = gpu.scenes.town_scene(60_000)
    gpu.pcd.write_pcd(tmp_path / "in.pcd", xyz, mode="binary")
    lines = dict(VGS_LINES if method == 2 else SVGS_LINES)
    lines.update({12: str(tmp_path) + "/", 15: "in.pcd", 18: str(tmp_path) + "/", 21: "out.pcd"})
    _write_task(tmp_path / "task.txt", method, lines)
    eng = gpu.Engine(gpu.default_params(method))
    eng.set_points(xyz)
    eng.run()
    plain = eng.point_labels()
    for flags, kw in (([], {}), (["--patch-radius", "0.1", "--switch-ratio", "0.5", "--no-fill"], dict(patch_radius=0.1, switch_ratio=0.5, fill=False))):
        out = subprocess.check_output([RUN, str(tmp_path / "task.txt"), "--seed", "4", "--refine"] + flags, text=True).split()
        eng.refine_labels(**kw)
        ref = eng.refined_labels()
        assert not np.array_equal(ref, plain)
        order, off = _grouping(ref)
        assert int(out[5]) == eng.counts()["kept"] == len(off) - 1 and int(out[6]) == order.size
        f, hdr = gpu.pcd.read_pcd(tmp_path / "out.pcd")
        assert int(hdr["POINTS"][0]) == order.size
        got = np.stack([f["x"], f["y"], f["z"]], axis=1)
        assert np.array_equal(got.view(np.uint32), xyz[order].view(np.uint32))
        rgb = f["rgb"].view(np.uint32)
        colours = [set(rgb[off[k]:off[k + 1]].tolist()) for k in range(len(off) - 1) if off[k + 1] > off[k]]
        assert all(len(c) == 1 for c in colours)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_refine_flags_usage_errors(tmp_path):
    """Argument parsing only: no device needed."""
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    for args, msg in ((["--no-fill"], b"need --refine"), (["--patch-radius", "0.1"], b"need --refine"),
                      (["--refine", "--switch-ratio", "2"], b"in [0, 1]"), (["--refine", "--patch-radius", "-1"], b"not negative"),
                      (["--refine", "--patch-radius", "nan"], b"not negative")):
        r = subprocess.run([RUN, str(tmp_path / "none.txt")] + args, capture_output=True)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr)
