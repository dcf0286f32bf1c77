#!/usr/bin/env python3
"""Time the tables of a per-point labelling of the tiled driver (NativeTiles.describe_labels, label_boxes and compare_labels(ref,
labels=...): vgs_tiles_point_label_descriptors, _boxes and vgs_tiles_compare_point_labels) on scenes.tiled_urban_scene, ranks as threads of
one process over LocalGroup on one GPU.  The labelling is the rank's refined labels (refine_labels() once, untimed), a torch tensor on the
device, read in place.  Per layout and rank: the wall time of the (always collective) descriptor call split into the rank's own records on
its GPU, the all-gather, the host fold and the algebra on its GPU (vgs_tiles_get_point_label_times), the same split for the box call (both
of its collectives added), the phases of the compare (vgs_tiles_get_compare_times), and the rank's payload
(vgs_tiles_get_point_label_payload: its moment records, its pair records and the bytes it put into the all-gather, header included).  The
reference ids are those of tools/tiles_segcompare_time.py.  The stages run once, untimed.  The median over the repeats after one warm-up
call is printed, one JSON line per layout.
usage: tools/tiles_labeldesc_time.py [points per rank] [repeats] [layouts, e.g. 2x2,4x2]"""
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vgs_svgs_segmentation_amd as v  # noqa: E402
from tiles_segcompare_time import reference_ids  # noqa: E402
from vgs_svgs_segmentation_amd import tiles_native as tn  # noqa: E402


def _timed(repeats, call, clock):
    call()   # the first call allocates the buffers
    wall, rows = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        rows.append(clock())
    return float(np.median(wall)), {k: float(np.median([x[k] for x in rows])) for k in rows[0]}


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
                counts = t.refine_labels()
                fine = torch.from_numpy(t.refined_labels().copy()).to("cuda:0")
                ref = torch.from_numpy(reference_ids(parts[r], labels)).to("cuda:0")
                d_wall, d_ms = _timed(repeats, lambda: t.describe_labels(fine, kept), t.point_label_times)
                pay = t.point_label_payload()
                b_wall, b_ms = _timed(repeats, lambda: t.label_boxes(fine, "principal", kept), t.point_label_times)
                box_bytes = t.point_label_payload()["bytes_sent"]
                c_wall, c_ms = _timed(repeats, lambda: t.compare_labels(ref, labels=fine, K=kept), t.compare_times)
                d = t.describe_labels(fine, kept)
                out[r] = dict(rank=r, kept=kept, points=int(parts[r].shape[0]), refined_filled=counts["points_filled"],
                              refined_changed=counts["points_changed"], labelled=int(d["n_points"].sum()), n_skipped=d["n_skipped"],
                              describe_ms=d_ms, describe_call_ms=d_wall, boxes_ms=b_ms, boxes_call_ms=b_wall, boxes_bytes_sent=box_bytes,
                              compare_ms=c_ms, compare_call_ms=c_wall, compare_payload=t.compare_payload(), **pay)
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
    layouts = sys.argv[3] if len(sys.argv) > 3 else "4x2"
    for lay in layouts.split(","):
        tx, ty = (int(x) for x in lay.split("x"))
        print(json.dumps(run_layout((tx, ty), n_per, repeats)), flush=True)


if __name__ == "__main__":
    main()
