#!/usr/bin/env python3
"""Time the tables of a per-point labelling (csrc/pointseg.hip) on URB10M with VGS (config 3): describe the refined labels, read in place
on the device (vgs_point_label_descriptors_device over vgs_get_refined_labels_device), and score them against a reference labelling
(Engine.compare_labels(ref, labels=refined), host arrays: two uploads included) -- beside what the node pass costs on the same engine,
the first segment_descriptors_device() after a run (csrc/segdesc.hip sorts V nodes, this pass N points).  Every time is wall-clock
around a call that ends with a stream synchronisation (launches, read-backs and the copy of the K rows included); the first call of each
kind allocates the buffers and is left out; the medians and their ratio go to stdout as one JSON line.
usage: tools/labeldesc_time.py [points] [repeats]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vgs_svgs_segmentation_amd as v  # noqa: E402


def describe_in_place(eng, ptr, n, K):
    """Engine.describe_labels without a torch tensor around the device pointer"""
    out = {name: np.zeros((K, w) if w > 1 else K, dtype=dt) for name, dt, w in v.Engine.DESCRIPTOR_FIELDS}
    skipped = C.c_int64(0)
    eng._ck(eng._L.vgs_point_label_descriptors_device(eng._h, C.c_void_p(ptr), n, K, C.byref(skipped),
                                                      *(out[name].ctypes.data_as(C.c_void_p) for name, _, _ in v.Engine.DESCRIPTOR_FIELDS)))
    return out, int(skipped.value)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    xyz = v.scenes.urban_scene(n)
    # a reference labelling with the grain of instances: one id per 4 m cell of the ground plan, a tenth of the points without annotation
    cell = np.floor(xyz[:, :2].astype(np.float64) / 4.0).astype(np.int64)
    cell -= cell.min(axis=0)
    ref = (cell[:, 0] * (int(cell[:, 1].max()) + 1) + cell[:, 1]).astype(np.int32)
    ref[::10] = -1
    eng = v.Engine(v.default_params(2, voxel_size=0.1))
    eng.set_points(xyz)
    node, desc, comp = [], [], []
    for it in range(reps + 1):
        eng.run()
        t = time.perf_counter()
        eng.segment_descriptors_device()
        t_node = (time.perf_counter() - t) * 1e3
        counts = eng.refine_labels()
        K = eng.counts()["kept"]
        ptr = eng.refined_labels_device_ptr()
        t = time.perf_counter()
        d, skipped = describe_in_place(eng, ptr, n, K)
        t_desc = (time.perf_counter() - t) * 1e3
        refined = eng.refined_labels()
        t = time.perf_counter()
        c = eng.compare_labels(ref, labels=refined)
        t_comp = (time.perf_counter() - t) * 1e3
        if it > 0:   # the first call of each kind allocates the buffers
            node.append(t_node); desc.append(t_desc); comp.append(t_comp)
    assert int(d["n_points"].sum()) == int((refined >= 0).sum()) - skipped
    cnt = eng.counts()
    med = lambda a: float(np.median(a))   # noqa: E731
    print(json.dumps(dict(config="c3", points=int(n), finite=cnt["finite"], nodes=cnt["voxels"], segments=K, largest=int(d["n_points"].max()) if K else 0,
                          refined_filled=counts["points_filled"], refined_changed=counts["points_changed"], cells=int(c["summary"][4]),
                          describe_labels_ms_median=med(desc), describe_labels_ms_min=float(np.min(desc)),
                          compare_labels_ms_median=med(comp), compare_labels_ms_min=float(np.min(comp)),
                          segment_descriptors_first_ms_median=med(node), segment_descriptors_first_ms_min=float(np.min(node)),
                          describe_over_segment_descriptors=med(desc) / med(node), repeats=reps, step_ms=eng.stage_times()["total"])), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
