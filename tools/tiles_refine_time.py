#!/usr/bin/env python3
"""Time the point-level label refinement of the tiled driver (NativeTiles.refine_labels: vgs_tiles_refine_point_labels) on
scenes.tiled_urban_scene, ranks as threads of one process over LocalGroup on one GPU.  Per layout and rank, with fill and without: the
wall time of the (always collective) call split into the rank's own band records on its GPU, the all-gather, the halo table and the
refinement on its GPU (vgs_tiles_get_refine_times), the rank's payload (vgs_tiles_get_refine_payload: the band records and the bytes it
put into the all-gather, header included) and its counts.  The band travels with the first call after a run only, so every repeat runs the
stages first (untimed) and times that first call: the figure is what a caller pays once per run.  "repeat_ms" is a second call behind
it, which sends the header alone.  The median over the repeats is printed, one JSON line per layout.
usage: tools/tiles_refine_time.py [points per rank] [repeats] [layouts, e.g. 2x2,4x2]"""
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
                res = dict(rank=r, points=int(parts[r].shape[0]))
                for key, fill in (("fill", True), ("nofill", False)):
                    rows, wall, again = [], [], []
                    for _ in range(repeats + 1):                      # (the first round warms up and is dropped)
                        t.run()
                        t0 = time.perf_counter()
                        counts = t.refine_labels(fill=fill)
                        wall.append((time.perf_counter() - t0) * 1e3)
                        rows.append(t.refine_times())
                        pay = t.refine_payload()
                        t0 = time.perf_counter()
                        t.refine_labels(fill=fill)
                        again.append((time.perf_counter() - t0) * 1e3)
                    res[key] = dict(ms={k: float(np.median([x[k] for x in rows[1:]])) for k in tn.R_NAMES}, call_ms=float(np.median(wall[1:])),
                                    repeat_ms=float(np.median(again[1:])), counts=counts, **pay)
                res["kept"] = t.point_labels()[1]
                out[r] = res
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
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    layouts = sys.argv[3] if len(sys.argv) > 3 else "4x2"
    for lay in layouts.split(","):
        tx, ty = (int(x) for x in lay.split("x"))
        print(json.dumps(run_layout((tx, ty), n_per, repeats)), flush=True)


if __name__ == "__main__":
    main()
