#!/usr/bin/env python3
"""Time the oriented boxes of the tiled driver (NativeTiles.segment_boxes: vgs_tiles_get_segment_boxes) on scenes.tiled_urban_scene,
ranks as threads of one process over LocalGroup on one GPU.  Per layout, rank and frame: the wall time of the first (collective) call
split into the rank's own extents on its GPU, the all-gather, the host fold and the finish on its GPU (vgs_tiles_get_box_times), and this
rank's payload (its extent records plus the header, 56 bytes each).  The descriptor table is taken first, so the box call holds the box
collective alone, and its phases (vgs_tiles_get_descriptor_times) are printed beside the boxes': own moments and own extents are one trip
each over the same points of the same rank.  The tables are cached per run, so every repeat runs the stages first (untimed); the median
over the repeats is printed, one JSON line per layout.
usage: tools/tiles_segbox_time.py [points per rank] [repeats] [layouts, e.g. 2x2,4x2]"""
import json
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vgs_svgs_segmentation_amd as v  # noqa: E402
from vgs_svgs_segmentation_amd import tiles_native as tn  # noqa: E402

FRAMES = ("principal", "upright")


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
                rows = {f: [] for f in FRAMES}
                drows = []
                for _ in range(repeats):
                    t.run()
                    d = t.segment_descriptors()
                    drows.append(t.descriptor_times())
                    for f in FRAMES:
                        t.segment_boxes(f)
                        rows[f].append(t.box_times())
                _, kept = t.point_labels()
                n_rec = len(t.own_segment_extents(kept, "principal", d)["label"])
                med = lambda xs, names: {k: float(np.median([x[k] for x in xs])) for k in names}  # noqa: E731
                out[r] = dict(rank=r, kept=kept, records=n_rec, payload_bytes=56 * (n_rec + 1),
                              ms={f: med(rows[f], tn.B_NAMES) for f in FRAMES}, descriptor_ms=med(drows, tn.D_NAMES))
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
