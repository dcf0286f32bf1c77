#!/usr/bin/env python3
"""Time the point-level label refinement (Engine.refine_labels: csrc/refine.hip) on URB10M with VGS (config 3) and with SVGS (config 4):
wall-clock around the call, which ends with a read-back of the counts (launches, the scans' read-backs and, for VGS with fill, the
adjacency rows of the unused voxels included), with fill and without, next to the oriented-box pass's first request in the same run for
scale.  The refinement is computed on every call; the box table is cached per run, so every repeat runs the stages first (untimed).
Prints one JSON line per configuration.
usage: tools/refine_time.py [points] [repeats]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vgs_svgs_segmentation_amd as v  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    xyz = v.scenes.urban_scene(n)
    for cfg, p in (("c3", v.default_params(2, voxel_size=0.1)), ("c4", v.default_params(3))):
        eng = v.Engine(p)
        eng.set_points(xyz)
        ms = {"refine_fill": [], "refine_nofill": [], "segbox": []}
        counts = {}
        for it in range(reps + 1):
            eng.run()
            dt = {}
            for key, fill in (("refine_fill", True), ("refine_nofill", False)):
                t = time.perf_counter()
                counts[key] = eng.refine_labels(fill=fill)
                dt[key] = (time.perf_counter() - t) * 1e3
            eng.segment_descriptors_device()
            t = time.perf_counter()
            eng.segment_boxes_device("principal")
            dt["segbox"] = (time.perf_counter() - t) * 1e3
            if it > 0:   # the first calls allocate the buffers
                for k in ms:
                    ms[k].append(dt[k])
        c = eng.counts()
        plain = eng.point_labels()
        eng.refine_labels()
        ref = eng.refined_labels()
        out = dict(config=cfg, points=int(n), nodes=c["voxels"], used=c["used"], segments=c["kept"], step_ms=eng.stage_times()["total"],
                   unlabelled_before=int((plain < 0).sum()), unlabelled_after=int((ref < 0).sum()))
        for key in ("refine_fill", "refine_nofill"):
            out[key + "_counts"] = counts[key]
        for k in ms:
            out[k + "_ms_median"] = float(np.median(ms[k]))
            out[k + "_ms_min"] = float(np.min(ms[k]))
        print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
