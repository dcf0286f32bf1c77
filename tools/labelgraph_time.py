#!/usr/bin/env python3
"""Time the adjacency graph of a per-point labelling (csrc/labelgraph.hip) on an urban scene with VGS (voxel_size 0.1; 10 M points is the
benchmark scene, config 3): one vgs_point_label_graph_device call over the engine's own point labels and one over the refined labels, both
read in place on the device, beside an uncached segment_graph_device() of the same engine and the same run -- the node pass, which does
strictly less work (no point sort, no vertex list, one label per node).  Every time is wall-clock around a call that ends with a stream
synchronisation (launches and read-backs included, the tables stay in HBM).  The segment graph is cached per run, so every repeat runs
the stages and the refinement first (untimed); the first repeat allocates the buffers and is left out.  The medians and their ratios go
to stdout as one JSON line.
usage: tools/labelgraph_time.py [points] [repeats]"""
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
    xyz = v.scenes.urban_scene(n)
    eng = v.Engine(v.default_params(2, voxel_size=0.1))
    eng.set_points(xyz)
    E, skipped = C.c_int64(0), C.c_int64(0)
    times = {"segment_graph": [], "own": [], "refined": []}
    edges = {}

    def graph(ptr, k):
        eng._ck(eng._L.vgs_point_label_graph_device(eng._h, C.c_void_p(ptr), n, k, C.byref(E), C.byref(skipped)))
        return int(E.value)

    for it in range(reps + 1):
        eng.run()
        counts = eng.refine_labels()
        K = eng.counts()["kept"]
        t = time.perf_counter()
        edges["segment_graph"], _ = eng.segment_graph_device()
        dt = {"segment_graph": (time.perf_counter() - t) * 1e3}
        for name, ptr in (("own", eng.point_labels_device_ptr()), ("refined", eng.refined_labels_device_ptr())):
            t = time.perf_counter()
            edges[name] = graph(ptr, K)
            dt[name] = (time.perf_counter() - t) * 1e3
        if it > 0:   # the first repeat allocates the buffers
            for name in times:
                times[name].append(dt[name])
    assert edges["own"] == edges["segment_graph"], edges
    g = eng.label_graph(eng.refined_labels(), K)
    c = eng.counts()
    med = {name: float(np.median(t)) for name, t in times.items()}
    print(json.dumps(dict(points=int(n), finite=c["finite"], nodes=c["voxels"], used=c["used"], segments=int(K), repeats=reps,
                          refined_filled=counts["points_filled"], refined_changed=counts["points_changed"], edges=edges,
                          refined_shared_nodes=int(g["n_shared"].sum()), refined_contacts=int(g["n_pairs"].sum()),
                          segment_graph_ms_median=med["segment_graph"], segment_graph_ms_min=float(np.min(times["segment_graph"])),
                          label_graph_own_ms_median=med["own"], label_graph_own_ms_min=float(np.min(times["own"])),
                          label_graph_refined_ms_median=med["refined"], label_graph_refined_ms_min=float(np.min(times["refined"])),
                          own_over_segment_graph=med["own"] / med["segment_graph"], refined_over_segment_graph=med["refined"] / med["segment_graph"],
                          step_ms=eng.stage_times()["total"])), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
