#!/usr/bin/env python3
"""Time absorbing the small parts of a per-point labelling (csrc/labelabsorb.hip) on an urban scene with VGS (voxel_size 0.1; 10 M points
is the benchmark scene, config 3), over the refined labels read in place on the device.  Beside it, in the same run on the same
labelling, the two passes a round is made of: vgs_point_label_components_device over the refined labels and
vgs_point_label_graph_device over THEIR PARTS (part_of_point with K = the number of parts: what a round runs), and for orientation the
graph of the refined labels themselves (the figure of tools/labelgraph_time.py).
One applied round = the call with max_rounds = 1 minus the call with max_rounds = 0: the latter is one evaluation without the graph
(parts, candidate flags), the former adds the graph of the parts, the targets, the relabelling -- and its final evaluation runs on the
relabelled points.  remainder = that round minus the two passes: what the new kernels, their sort and their read-backs cost.  The call
with the default cap (8) gives the rounds the scene needs.
Every time is wall-clock around a call that ends with a stream synchronisation (launches and read-backs included, the results stay in
HBM); the first repeat allocates the buffers and is left out; medians, minima and maxima go to stdout as one JSON line.
usage: tools/labelabsorb_time.py [points] [repeats] [min_points] [island_points]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vgs_svgs_segmentation_amd as v  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    min_points = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    island_points = int(sys.argv[4]) if len(sys.argv) > 4 else 500
    xyz = v.scenes.urban_scene(n)
    eng = v.Engine(v.default_params(2, voxel_size=0.1))
    eng.set_points(xyz)
    eng.run()
    refine = eng.refine_labels()
    K = eng.counts()["kept"]
    ptr = C.c_void_p(eng.refined_labels_device_ptr())
    a, b = C.c_int64(0), C.c_int64(0)
    counts = np.zeros(8, dtype=np.int64)
    info = {}

    def components():
        eng._ck(eng._L.vgs_point_label_components_device(eng._h, ptr, n, K, C.byref(a), C.byref(b)))
        info["parts"] = int(a.value)

    def graph_of_parts():   # (behind components(): the parts are in HBM)
        pop = eng.label_components_device()["part_of_point"]
        eng._ck(eng._L.vgs_point_label_graph_device(eng._h, C.c_void_p(pop), n, info["parts"], C.byref(a), C.byref(b)))
        info["part_edges"] = int(a.value)

    def graph():
        eng._ck(eng._L.vgs_point_label_graph_device(eng._h, ptr, n, K, C.byref(a), C.byref(b)))
        info["edges"] = int(a.value)

    def absorb(max_rounds):
        def call():
            ap = v._lib.AbsorbParams(min_points, island_points, max_rounds, 0)
            eng._ck(eng._L.vgs_absorb_point_label_parts_device(eng._h, ptr, n, K, C.byref(ap), counts.ctypes.data_as(C.c_void_p)))
            info["absorb_%d" % max_rounds] = dict(zip(v.Engine.ABSORB_COUNTS, (int(x) for x in counts)))
        return call

    calls = (("components", components), ("graph_of_parts", graph_of_parts), ("graph_of_labels", graph), ("absorb_0", absorb(0)),
             ("absorb_1", absorb(1)), ("absorb_8", absorb(8)))
    times = {name: [] for name, _ in calls}
    for it in range(reps + 1):
        for name, fn in calls:
            t = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t) * 1e3
            if it > 0:   # the first repeat allocates the buffers
                times[name].append(dt)
    med = {name: float(np.median(t)) for name, t in times.items()}
    rounds = [t1 - t0 for t0, t1 in zip(times["absorb_0"], times["absorb_1"])]
    one_round = float(np.median(rounds))
    c = eng.counts()
    print(json.dumps(dict(points=int(n), finite=c["finite"], nodes=c["voxels"], used=c["used"], segments=int(K), repeats=reps,
                          refined_filled=refine["points_filled"], refined_changed=refine["points_changed"], min_points=min_points,
                          island_points=island_points, parts=info["parts"], part_edges=info["part_edges"], edges=info["edges"],
                          ms_median=med, ms_min={k: float(np.min(t)) for k, t in times.items()}, ms_max={k: float(np.max(t)) for k, t in times.items()},
                          round_ms_median=one_round, round_ms_min=float(np.min(rounds)), round_ms_max=float(np.max(rounds)),
                          remainder_ms=one_round - med["components"] - med["graph_of_parts"],
                          counts={k: info[k] for k in ("absorb_0", "absorb_1", "absorb_8")}, step_ms=eng.stage_times()["total"])), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
