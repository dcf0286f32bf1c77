#!/usr/bin/env python3
"""Time the segment adjacency graph of the tiled driver (NativeTiles.segment_graph: vgs_tiles_get_segment_graph) on
scenes.tiled_urban_scene, ranks as threads of one process over LocalGroup on one GPU.  Per layout and rank: the wall time of the first
(collective) call split into the halo labels (list and upload), the rank's own table on its GPU, the all-gather and the host fold
(vgs_tiles_get_graph_times), and this rank's payload (halo labels handed to its context; its edge records plus the header, 48 bytes
each).  The table is cached per run, so every repeat runs the stages first (untimed); the median over the repeats is printed, one JSON
line per layout.  The contexts share one device, so the exchange figure is mostly a wait for the slowest rank.
usage: tools/tiles_seggraph_time.py [points per rank] [repeats] [layouts, e.g. 2x2,4x2]"""
import json
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vgs_svgs_segmentation_amd as v  # noqa: E402
from vgs_svgs_segmentation_amd import tiles_native as tn  # noqa: E402


def run_layout(tiles, n_per, repeats):
    world = tiles[0] * tiles[1]
    pitch = 50.0 * np.sqrt(n_per / 10_000_000)
    parts = [v.scenes.tiled_urban_scene(n_per * world, tiles=tiles, tile_index=r) for r in range(world)]
    grp = tn.LocalGroup(world)
    out = [None] * world

    def rank_main(r):
        try:
            t = tn.NativeTiles(v.default_params(2, voxel_size=0.1), tn.COMM_LOCAL, grp.handle, r, world, tiles, pitch)
            try:
                t.set_points(parts[r])
                rows = []
                for _ in range(repeats):
                    t.run()
                    edges = t.segment_graph()["seg_ab"].shape[0]
                    rows.append(t.graph_times())
                _, kept = t.point_labels()
                p = t.graph_payload()
                out[r] = dict(rank=r, kept=kept, edges=edges, halo_labels=p["halo_labels"], records=p["own_edges"], payload_bytes=p["bytes_sent"],
                              ms={k: float(np.median([x[k] for x in rows])) for k in tn.G_NAMES})
            finally:
                t.close()
        except Exception as ex:  # noqa: BLE001
            out[r] = repr(ex)
            grp.abort()
    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(1800)
    grp.close()
    return dict(layout=f"{tiles[0]}x{tiles[1]}", points_per_rank=n_per, repeats=repeats, ranks=out)


def main():
    n_per = int(sys.argv[1]) if len(sys.argv) > 1 else 2_500_000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    layouts = sys.argv[3] if len(sys.argv) > 3 else "2x2,4x2"
    for lay in layouts.split(","):
        tx, ty = (int(x) for x in lay.split("x"))
        print(json.dumps(run_layout((tx, ty), n_per, repeats)), flush=True)


if __name__ == "__main__":
    main()
