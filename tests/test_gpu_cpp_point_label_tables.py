"""The C++ mirror of the point-labelling tables (include/vgs_segmentation.hpp: getLabelDescriptors, getLabelBoxes and
compareClusterLabels(ref, n, labels) on both classes) through vgs_run --refine --refined-segments / --refined-segment-boxes /
--refined-matches / --refined-truth-matches, against Engine.describe_labels / label_boxes / compare_labels(labels=) over
Engine.refined_labels() for the same task, by value: the CSVs read back exactly.  The voxel-label files of the same invocation stay what
they are without the new flags."""
import subprocess

import numpy as np
import pytest

from test_cpp_segment_desc import CSRC, RUN, SVGS_LINES, VGS_LINES, _write_task


def _rows(path, width):
    rows = np.loadtxt(path, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    assert rows.shape[1] == width, path
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("method", [2, 3], ids=["vgs", "svgs"])
def test_refined_csvs_match_the_engine(gpu, tmp_path, method):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    xyz = gpu.scenes.town_scene(60_000)
    truth = (np.arange(xyz.shape[0]) // 53 % 41 - 2).astype(np.int32)
    gpu.pcd.write_pcd(tmp_path / "in.pcd", xyz, mode="binary", extra={"instance": truth})
    lines = dict(VGS_LINES if method == 2 else SVGS_LINES)
    lines.update({12: str(tmp_path) + "/", 15: "in.pcd", 18: str(tmp_path) + "/", 21: "out.pcd"})
    task = str(tmp_path / "task.txt")
    _write_task(task, method, lines)
    f = {n: tmp_path / (n + ".csv") for n in ("seg0", "box0", "m0", "seg", "box", "m", "t", "rseg", "rbox", "rbox_up", "rm", "rt")}
    subprocess.check_call([RUN, task, "--refine", "--segments", str(f["seg0"]), "--segment-boxes", str(f["box0"]), "--segment-matches", str(f["m0"]),
                           "--truth-field", "instance"], stdout=subprocess.DEVNULL)
    out = subprocess.check_output([RUN, task, "--refine", "--segments", str(f["seg"]), "--segment-boxes", str(f["box"]), "--segment-matches", str(f["m"]),
                                   "--truth-field", "instance", "--truth-matches", str(f["t"]), "--refined-segments", str(f["rseg"]),
                                   "--refined-segment-boxes", str(f["rbox"]), "--refined-matches", str(f["rm"]), "--refined-truth-matches", str(f["rt"])],
                                  text=True).splitlines()
    subprocess.check_call([RUN, task, "--refine", "--refined-segment-boxes", str(f["rbox_up"]), "--box-frame", "upright"], stdout=subprocess.DEVNULL)
    for a, b in (("seg", "seg0"), ("box", "box0"), ("m", "m0")):   # the voxel-label tables do not depend on the new flags
        assert f[a].read_bytes() == f[b].read_bytes(), a
    eng = gpu.Engine(gpu.default_params(method))
    eng.set_points(xyz)
    eng.run()
    eng.refine_labels()
    refined = eng.refined_labels()
    K = eng.counts()["kept"]
    d = eng.describe_labels(refined)
    rows = _rows(f["rseg"], 29)
    assert rows.shape[0] == K and np.array_equal(rows[:, 0], np.arange(K))
    assert np.array_equal(rows[:, 1].astype(np.int64), d["n_points"]) and np.array_equal(rows[:, 2].astype(np.int32), d["n_nodes"])
    assert np.array_equal(rows[:, 3:9].astype(np.float32), d["bbox6"])
    assert np.array_equal(rows[:, 9:12], d["centroid3"]) and np.array_equal(rows[:, 12:15], d["evals3"])
    V = d["evecs9"].reshape(K, 3, 3)
    assert np.array_equal(rows[:, 15:18], V[:, :, 0]) and np.array_equal(rows[:, 18:21], V[:, :, 2])
    assert np.array_equal(rows[:, 21:29].astype(np.float32), d["eigen8"])
    assert not np.array_equal(rows[:, 1], _rows(f["seg"], 29)[:, 1])   # (another labelling than the voxel labels')
    for path, frame in ((f["rbox"], "principal"), (f["rbox_up"], "upright")):
        b, rows = eng.label_boxes(refined, frame), _rows(path, 22)
        want = np.concatenate([b["center3"], b["half3"], b["frame9"], b["lo3"], b["hi3"]], axis=1)
        assert rows.shape[0] == K and np.array_equal(rows[:, 1:], want), frame
    c = eng.compare_labels(truth, labels=refined)
    rows = _rows(f["rm"], 6)
    want = np.stack([np.arange(K), c["seg_annotated"], c["seg_refs"], c["seg_best_ref"], c["seg_best_n"], c["seg_best_iou"]], axis=1).astype(np.float64)
    assert np.array_equal(rows, want)
    rows = _rows(f["rt"], 6)
    want = np.stack([c["ref_id"], c["ref_points"], c["ref_dropped"], c["ref_best_seg"], c["ref_best_n"], c["ref_best_iou"]], axis=1).astype(np.float64)
    assert np.array_equal(rows, want)
    line = [ln for ln in out if ln.startswith("refined-matches ")]
    assert len(line) == 1 and [int(v) for v in line[0].split()[1:]] == c["summary"].tolist()
    assert sum(ln.startswith("refined-scores ") for ln in out) == 1 and sum(ln.startswith("matches ") for ln in out) == 1
