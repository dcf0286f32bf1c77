#!/usr/bin/env python3
"""Time the attribute tables of a per-point labelling of the tiled driver (NativeTiles.label_field_stats and label_class_histogram:
vgs_tiles_point_label_field_stats, vgs_tiles_point_label_class_histogram) on scenes.tiled_urban_scene, ranks as threads of one process
over LocalGroup on one GPU.  The labelling is the rank's refined labels (refine_labels() once, untimed); labels, fields and classes are
torch tensors on the device, read in place.  Per layout and rank, for fields of 1, 4 and 16 channels and for 16 classes: the wall time of
the (always collective) call split into the rank's own records on its GPU, the all-gather, the host fold and the finish on its GPU
(vgs_tiles_get_field_times), and the rank's payload (vgs_tiles_get_field_payload: its records and the bytes it put into the all-gather,
header included).  Beside them, as the yardstick, the node tables over the same tensors (segment_field_stats, segment_class_histogram).
The stages run once, untimed.  The median over the repeats after one warm-up call is printed, one JSON line per layout.
usage: tools/tiles_labelfield_time.py [points per rank] [repeats] [layouts, e.g. 2x2,4x2]"""
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vgs_svgs_segmentation_amd as v  # noqa: E402
from vgs_svgs_segmentation_amd import tiles_native as tn  # noqa: E402

CHANNELS = (1, 4, 16)
N_CLASSES = 16


def _timed(repeats, call, clock, payload):
    call()   # the first call allocates the buffers
    wall, rows = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        rows.append(clock())
    return dict(call_ms=float(np.median(wall)), **{k + "_ms": float(np.median([x[k] for x in rows])) for k in rows[0]}, **payload())


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
                n = parts[r].shape[0]
                t.set_points(parts[r])
                t.run()
                _, kept = t.point_labels()
                counts = t.refine_labels()
                fine = torch.from_numpy(t.refined_labels().copy()).to("cuda:0")
                rng = np.random.default_rng(100 + r)
                cls = torch.from_numpy(rng.integers(-1, N_CLASSES + 1, n).astype(np.int32)).to("cuda:0")
                res = dict(rank=r, kept=kept, points=int(n), refined_filled=counts["points_filled"], refined_changed=counts["points_changed"])
                for ch in CHANNELS:
                    f = torch.from_numpy(rng.normal(100.0, 7.0, (n, ch)).astype(np.float32)).to("cuda:0")
                    res[f"label_fields_{ch}"] = _timed(repeats, lambda: t.label_field_stats(fine, f, kept), t.field_times, t.field_payload)
                    res[f"segment_fields_{ch}"] = _timed(repeats, lambda: t.segment_field_stats(f), t.field_times, t.field_payload)
                res["label_classes"] = _timed(repeats, lambda: t.label_class_histogram(fine, cls, N_CLASSES, kept), t.field_times, t.field_payload)
                res["segment_classes"] = _timed(repeats, lambda: t.segment_class_histogram(cls, N_CLASSES), t.field_times, t.field_payload)
                s = t.label_class_histogram(fine, cls, N_CLASSES, kept)
                res["labelled"], res["n_skipped"] = int(s["hist"].sum() + s["n_outside"].sum()), s["n_skipped"]
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
    return dict(layout=f"{tiles[0]}x{tiles[1]}", points_per_rank=n_per, repeats=repeats, channels=list(CHANNELS), n_classes=N_CLASSES, ranks=out)


def main():
    n_per = int(sys.argv[1]) if len(sys.argv) > 1 else 2_500_000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    layouts = sys.argv[3] if len(sys.argv) > 3 else "4x2"
    for lay in layouts.split(","):
        tx, ty = (int(x) for x in lay.split("x"))
        print(json.dumps(run_layout((tx, ty), n_per, repeats)), flush=True)


if __name__ == "__main__":
    main()
