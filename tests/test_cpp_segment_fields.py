"""vgs_run --segment-fields / --segment-classes: the attribute CSVs of the task-file front end (read_pcd_fields of
include/point_clouds_io.hpp -> examples/drivers.hpp -> getClusterFieldStats / getClusterClassHistogram of include/vgs_segmentation.hpp)
against Engine.segment_field_stats / segment_class_histogram for the same task, by value; the --segments file of the same invocation
against one written without the new flags; and the class-level getters before segmentation."""
import subprocess

import numpy as np
import pytest

from test_cpp_segment_desc import CSRC, RUN, SVGS_LINES, VGS_LINES, _write_task

N_CLASSES = 6


def _attributes(n):
    rng = np.random.default_rng(31)
    inten = rng.uniform(0.0, 1.0, n).astype(np.float32)
    inten[rng.choice(n, 50, replace=False)] = np.nan
    cls = rng.integers(0, N_CLASSES + 2, n).astype(np.uint8)      # two classes outside the histogram
    return inten, cls


@pytest.mark.gpu
@pytest.mark.parametrize("method", [2, 3], ids=["vgs", "svgs"])
def test_attribute_csvs_match_engine(gpu, tmp_path, method):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    xyz = gpu.scenes.town_scene(60_000)
    inten, cls = _attributes(xyz.shape[0])
    gpu.pcd.write_pcd(tmp_path / "in.pcd", xyz, mode="binary", extra={"intensity": inten, "cls": cls})
    lines = dict(VGS_LINES if method == 2 else SVGS_LINES)
    lines.update({12: str(tmp_path) + "/", 15: "in.pcd", 18: str(tmp_path) + "/", 21: "out.pcd"})
    _write_task(tmp_path / "task.txt", method, lines)
    plain, seg, fcsv, ccsv = (tmp_path / n for n in ("plain.csv", "segments.csv", "fields.csv", "classes.csv"))
    subprocess.check_call([RUN, str(tmp_path / "task.txt"), "--segments", str(plain)], stdout=subprocess.DEVNULL)
    subprocess.check_call([RUN, str(tmp_path / "task.txt"), "--segments", str(seg), "--segment-fields", str(fcsv), "--fields", "intensity,z",
                           "--segment-classes", str(ccsv), "--class-field", "cls", "--classes", str(N_CLASSES)], stdout=subprocess.DEVNULL)
    assert seg.read_bytes() == plain.read_bytes()   # the --segments file does not depend on the new flags
    eng = gpu.Engine(gpu.default_params(method))
    eng.set_points(xyz)
    eng.run()
    st = eng.segment_field_stats(np.stack([inten, xyz[:, 2]], axis=1))
    K = st["mean"].shape[0]
    assert K > 0 and (st["n_valid"][:, 0] < st["n_valid"][:, 1]).any()
    with open(fcsv) as f:
        header = f.readline().strip().split(",")
    assert header == ["label"] + [f"{n}_{s}" for n in ("intensity", "z") for s in ("n_valid", "mean", "var", "min", "max")]
    rows = np.loadtxt(fcsv, delimiter=",", skiprows=1, dtype=np.float64, ndmin=2)
    assert rows.shape == (K, 11) and np.array_equal(rows[:, 0], np.arange(K))
    for c in range(2):
        o = 1 + 5 * c
        assert np.array_equal(rows[:, o].astype(np.int64), st["n_valid"][:, c])
        # %.17g doubles and %.9g floats read back exactly
        assert np.array_equal(rows[:, o + 1], st["mean"][:, c], equal_nan=True) and np.array_equal(rows[:, o + 2], st["var"][:, c], equal_nan=True)
        assert np.array_equal(rows[:, o + 3].astype(np.float32), st["vmin"][:, c], equal_nan=True)
        assert np.array_equal(rows[:, o + 4].astype(np.float32), st["vmax"][:, c], equal_nan=True)
    h = eng.segment_class_histogram(cls.astype(np.int32), N_CLASSES)
    with open(ccsv) as f:
        header = f.readline().strip().split(",")
    assert header == ["label", "majority", "majority_count", "n_outside"] + [f"hist_{j}" for j in range(N_CLASSES)]
    rows = np.loadtxt(ccsv, delimiter=",", skiprows=1, dtype=np.int64, ndmin=2)
    assert rows.shape == (K, 4 + N_CLASSES) and np.array_equal(rows[:, 0], np.arange(K))
    assert np.array_equal(rows[:, 1], h["majority"]) and np.array_equal(rows[:, 2], h["majority_count"])
    assert np.array_equal(rows[:, 3], h["n_outside"]) and np.array_equal(rows[:, 4:], h["hist"])
    assert h["n_outside"].sum() > 0
    # a field the file does not have: an error that names it
    r = subprocess.run([RUN, str(tmp_path / "task.txt"), "--segment-fields", str(tmp_path / "no.csv"), "--fields", "reflectance"], capture_output=True)
    assert r.returncode == 1 and b"reflectance" in r.stderr


@pytest.mark.gpu
def test_class_getters_before_and_after_segmentation(gpu):
    """VoxelBasedSegmentation returns empty tables before drawColorMapofPointsinClusters, as getClusterBoxes does, and the engine's tables
    afterwards; SuperVoxelBasedSegmentation raises the state error until the cloud is segmented."""
    xyz = gpu.scenes.town_scene(60_000)
    inten, cls = _attributes(xyz.shape[0])
    cls = cls.astype(np.int32)
    v = gpu.VoxelBasedSegmentation(0.15)
    v.setInputCloud(xyz); v.getCloudPointNum(xyz); v.addPointsFromInputCloud()
    v.setVoxelSize(0.15, 10, 3, 3)
    v.setVoxelCenters(); v.calcualteVoxelCloudAttributes(xyz); v.findAllVoxelAdjacency(0.5)
    v.segmentVoxelCloudWithGraphModel(0.3, 0.2, 0.2, 0.2, 0.2, 0.2, 2.0)
    e = v.getClusterFieldStats(xyz)
    assert sorted(e) == sorted(n for n, _ in gpu.Engine.FIELD_STAT_FIELDS) and all(a.shape == (0, 3) for a in e.values())
    assert v.getClusterFieldStats(inten)["mean"].shape == (0, 1)
    e = v.getClusterClassHistogram(cls, N_CLASSES)
    assert e["hist"].shape == (0, N_CLASSES) and all(e[k].shape == (0,) for k in ("n_outside", "majority", "majority_count"))
    v.drawColorMapofPointsinClusters()
    a, b = v.getClusterFieldStats(inten), v.engine.segment_field_stats(inten)
    assert a["mean"].shape[0] == len(v.getClusterIdx()) > 0 and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)
    a, b = v.getClusterClassHistogram(cls, N_CLASSES), v.engine.segment_class_histogram(cls, N_CLASSES)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    s = gpu.SuperVoxelBasedSegmentation(0.05)
    s.setInputCloud(xyz); s.getCloudPointNum(xyz); s.addPointsFromInputCloud()
    for call in (lambda: s.getClusterFieldStats(inten), lambda: s.getClusterClassHistogram(cls, N_CLASSES)):
        with pytest.raises(gpu.VgsError) as err:
            call()
        assert err.value.status == gpu._lib.VGS_E_STATE
