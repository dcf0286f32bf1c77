#!/usr/bin/env python3
"""Time the oriented boxes of the kept segments (Engine.segment_boxes_device: csrc/segbox.hip) on URB10M with VGS (config 3) and with SVGS
(config 4): the first request for each frame after a run, with the descriptor table already cached, next to the descriptor pass's own
first request in the same run.  Times are wall-clock around the call, which ends with a stream synchronisation (launches included); the
tables are cached per run, so every repeat runs the stages first (untimed), and the frame asked for first alternates from repeat to
repeat.  Prints one JSON line per configuration.
usage: tools/segbox_time.py [points] [repeats]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vgs_svgs_segmentation_amd as v  # noqa: E402

FRAMES = ("principal", "upright")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    xyz = v.scenes.urban_scene(n)
    for cfg, p in (("c3", v.default_params(2, voxel_size=0.1)), ("c4", v.default_params(3))):
        eng = v.Engine(p)
        eng.set_points(xyz)
        ms = {"descriptors": [], "principal": [], "upright": []}
        for it in range(reps + 1):
            eng.run()
            t = time.perf_counter()
            eng.segment_descriptors_device()
            dt = {"descriptors": (time.perf_counter() - t) * 1e3}
            for f in (FRAMES if it % 2 else FRAMES[::-1]):
                t = time.perf_counter()
                eng.segment_boxes_device(f)
                dt[f] = (time.perf_counter() - t) * 1e3
            if it > 0:   # the first calls allocate the buffers
                for k in ms:
                    ms[k].append(dt[k])
        t = time.perf_counter()
        b = eng.segment_boxes("upright")
        copy_ms = (time.perf_counter() - t) * 1e3
        K = int(b["lo3"].shape[0])
        c = eng.counts()
        out = dict(config=cfg, points=int(n), nodes=c["voxels"], segments=K, cached_download_ms=copy_ms, step_ms=eng.stage_times()["total"])
        for k in ms:
            out[k + "_ms_median"] = float(np.median(ms[k]))
            out[k + "_ms_min"] = float(np.min(ms[k]))
        print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
