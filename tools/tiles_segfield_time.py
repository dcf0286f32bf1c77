#!/usr/bin/env python3
"""Time the attribute statistics of the tiled driver (NativeTiles.segment_field_stats / segment_class_histogram:
vgs_tiles_segment_field_stats, vgs_tiles_segment_class_histogram) on scenes.tiled_urban_scene, ranks as threads of one process over
LocalGroup on one GPU.  Per layout and rank, for fields of 1, 4 and 16 channels and a histogram of 16 classes: the wall time of the
(always collective) call split into the rank's own records on its GPU, the all-gather, the host fold and the finish on its GPU
(vgs_tiles_get_field_times), and the rank's payload (vgs_tiles_get_field_payload: its records and the bytes it put into the all-gather,
header included).  The inputs are torch tensors on the device, read in place, as in tools/segfield_time.py; the stages run once,
untimed.  The median over the repeats after one warm-up call is printed, one JSON line per layout.
usage: tools/tiles_segfield_time.py [points per rank] [repeats] [layouts, e.g. 2x2,4x2]"""
import json
import os
import sys
import threading

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vgs_svgs_segmentation_amd as v  # noqa: E402
from vgs_svgs_segmentation_amd import tiles_native as tn  # noqa: E402

CHANNELS = (1, 4, 16)
N_CLASSES = 16


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
                t.run()
                labels, kept = t.point_labels()
                n = parts[r].shape[0]
                rng = np.random.default_rng(5 + r)
                med = lambda xs: {k: float(np.median([x[k] for x in xs])) for k in tn.F_NAMES}  # noqa: E731
                calls = {}
                for ch in CHANNELS:
                    f = torch.from_numpy(rng.normal(100.0, 10.0, (n, ch)).astype(np.float32)).to("cuda:0")
                    t.segment_field_stats(f)
                    rows = []
                    for _ in range(repeats):
                        t.segment_field_stats(f)
                        rows.append(t.field_times())
                    calls[f"field_{ch}"] = dict(ms=med(rows), **t.field_payload())
                cls = torch.from_numpy(rng.integers(0, N_CLASSES, n).astype(np.int32)).to("cuda:0")
                t.segment_class_histogram(cls, N_CLASSES)
                rows = []
                for _ in range(repeats):
                    t.segment_class_histogram(cls, N_CLASSES)
                    rows.append(t.field_times())
                calls[f"hist_{N_CLASSES}"] = dict(ms=med(rows), **t.field_payload())
                out[r] = dict(rank=r, kept=kept, points=n, labelled=int((labels >= 0).sum()), calls=calls)
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
    layouts = sys.argv[3] if len(sys.argv) > 3 else "2x2"
    for lay in layouts.split(","):
        tx, ty = (int(x) for x in lay.split("x"))
        print(json.dumps(run_layout((tx, ty), n_per, repeats)), flush=True)


if __name__ == "__main__":
    main()
