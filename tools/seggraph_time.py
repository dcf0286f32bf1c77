#!/usr/bin/env python3
"""Time the segment adjacency graph (Engine.segment_graph_device: csrc/seggraph.hip) on URB10M with VGS (config 3) and with SVGS
(config 4), beside the host route a caller has without it for the neighbourhood part alone: vgs_get_lists(0) (the full adjacency lists),
the kept node labels, and numpy to join them into label pairs (no weights).  The device time is wall-clock around the call, which ends
with a stream synchronisation (launches included); the graph is cached per run, so every repeat runs the stages first (untimed).  Prints
one JSON line per configuration.
usage: tools/seggraph_time.py [points] [repeats]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vgs_svgs_segmentation_amd as v  # noqa: E402


def host_route(eng):
    """Edges and node-pair counts from the host getters: lists(0) + node labels + numpy."""
    off, idx = eng.lists("adjacency")
    _, kept = eng.node_labels()
    used = eng.attributes()["used"].astype(bool)
    lab = np.where(used, kept, -1).astype(np.int64)
    K = int(eng.counts()["kept"])
    u = np.repeat(np.arange(lab.shape[0], dtype=np.int64), np.diff(off))
    w = idx.astype(np.int64)
    m = (lab[u] >= 0) & (lab[w] >= 0) & (lab[u] != lab[w]) & (u < w)
    la, lb = lab[u[m]], lab[w[m]]
    keys = np.unique(np.minimum(la, lb) * K + np.maximum(la, lb))
    return keys.shape[0], int(idx.shape[0])


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
            E, _ = eng.segment_graph_device()
            dt = (time.perf_counter() - t) * 1e3
            if it > 0:   # the first call allocates the buffers
                dev.append(dt)
        t = time.perf_counter()
        g = eng.segment_graph()
        copy_ms = (time.perf_counter() - t) * 1e3
        c = eng.counts()
        t = time.perf_counter()
        E_host, n_list = host_route(eng)
        host_ms = (time.perf_counter() - t) * 1e3
        assert E_host == E, (E_host, E)
        records = int(g["nodes_ab"].astype(np.int64).sum())   # one record per (node, neighbour segment)
        print(json.dumps(dict(config=cfg, points=int(n), nodes=c["voxels"], used=c["used"], segments=int(c["kept"]), records=records, edges=int(E),
                              node_pairs=int(g["n_pairs"].sum()), device_ms_median=float(np.median(dev)), device_ms_min=float(np.min(dev)),
                              cached_download_ms=copy_ms, host_route_ms=host_ms, host_list_entries=n_list,
                              step_ms=eng.stage_times()["total"])), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
