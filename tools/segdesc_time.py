#!/usr/bin/env python3
"""Time the per-segment descriptors (Engine.segment_descriptors_device: csrc/segdesc.hip) on URB10M with VGS (config 3) and with SVGS
(config 4), beside the host path a caller has without them: download the labels, group the points with numpy (count, two-pass centroid,
covariance, box, eigh).  The device time is wall-clock around the call, which ends with a stream synchronisation (launches included); the
descriptors are cached per run, so every repeat runs the stages first (untimed).  Prints one JSON line per configuration.
usage: tools/segdesc_time.py [points] [repeats]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vgs_svgs_segmentation_amd as v  # noqa: E402


def host_path(eng, xyz, K):
    labels = eng.point_labels()
    m = labels >= 0
    lab = labels[m].astype(np.int64)
    x = xyz[m].astype(np.float64)
    n = np.bincount(lab, minlength=K)
    mean = np.stack([np.bincount(lab, x[:, a], minlength=K) for a in range(3)], axis=1) / n[:, None]
    d = x - mean[lab]
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    cov = np.stack([np.bincount(lab, d[:, i] * d[:, j], minlength=K) for i, j in pairs], axis=1) / n[:, None]
    order = np.argsort(lab, kind="stable")
    starts = np.concatenate([[0], np.cumsum(n)[:-1]])
    xs = xyz[m][order]
    np.minimum.reduceat(xs, starts, axis=0), np.maximum.reduceat(xs, starts, axis=0)
    M = np.empty((K, 3, 3))
    for c, (i, j) in enumerate(pairs):
        M[:, i, j] = cov[:, c]
        M[:, j, i] = cov[:, c]
    np.linalg.eigh(M)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    xyz = v.scenes.urban_scene(n)
    for cfg, p in (("c3", v.default_params(2, voxel_size=0.1)), ("c4", v.default_params(3))):
        eng = v.Engine(p)
        eng.set_points(xyz)
        dev = []
        for it in range(reps + 1):
            eng.run()
            t = time.perf_counter()
            eng.segment_descriptors_device()
            dt = (time.perf_counter() - t) * 1e3
            if it > 0:   # the first call allocates the buffers
                dev.append(dt)
        t = time.perf_counter()
        d = eng.segment_descriptors()
        copy_ms = (time.perf_counter() - t) * 1e3
        K = int(d["n_points"].shape[0])
        t = time.perf_counter()
        host_path(eng, xyz, K)
        host_ms = (time.perf_counter() - t) * 1e3
        c = eng.counts()
        print(json.dumps(dict(config=cfg, points=int(n), nodes=c["voxels"], segments=K, largest=int(d["n_points"].max()) if K else 0,
                              device_ms_median=float(np.median(dev)), device_ms_min=float(np.min(dev)), cached_download_ms=copy_ms,
                              host_numpy_ms=host_ms, step_ms=eng.stage_times()["total"])), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
