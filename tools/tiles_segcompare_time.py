#!/usr/bin/env python3
"""Time the label comparison of the tiled driver (NativeTiles.compare_labels: vgs_tiles_compare_labels) on scenes.tiled_urban_scene,
ranks as threads of one process over LocalGroup on one GPU.  Per layout and rank: the wall time of the (always collective) call split
into the rank's own cells on its GPU, the all-gather and the tables on its GPU (vgs_tiles_get_compare_times), and the rank's payload
(vgs_tiles_get_compare_payload: its cells and the bytes it put into the all-gather, header included).  The reference ids are torch tensors
on the device, read in place, as in tools/segcompare_time.py, and made per rank from its own points and labels: the segment's label in
every second 4 m column of the ground plan, a per-column id elsewhere, one point in 50 without annotation.  The stages run once, untimed.
Beside it the path the call replaces, timed in the same script: point_labels() on every rank (each rank's download, the slowest counts),
then tests/label_compare_ref.py's compare_labels (np.unique) over the concatenation on one host; its tables must equal the tiled ones.
The median over the repeats after one warm-up call is printed, one JSON line per layout.
usage: tools/tiles_segcompare_time.py [points per rank] [repeats] [layouts, e.g. 2x2,4x2]"""
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import label_compare_ref as R  # noqa: E402
import vgs_svgs_segmentation_amd as v  # noqa: E402
from vgs_svgs_segmentation_amd import tiles_native as tn  # noqa: E402


def reference_ids(xyz, labels):
    cx = np.floor(xyz[:, 0].astype(np.float64) / 4.0).astype(np.int64)
    cy = np.floor(xyz[:, 1].astype(np.float64) / 4.0).astype(np.int64)
    ids = np.where((cx + cy) % 2 == 0, labels.astype(np.int64), 1_000_000 + cx % 1000 + 1000 * (cy % 1000))
    ids[::50] = -1
    return np.ascontiguousarray(ids.astype(np.int32))


def run_layout(tiles, n_per, repeats):
    world = tiles[0] * tiles[1]
    pitch = 50.0 * np.sqrt(n_per / 10_000_000)
    parts = [v.scenes.tiled_urban_scene(n_per * world, tiles=tiles, tile_index=r) for r in range(world)]
    grp = tn.LocalGroup(world)
    out = [None] * world
    keep = [None] * world

    def rank_main(r):
        try:
            t = tn.NativeTiles(v.default_params(2, voxel_size=0.1), tn.COMM_LOCAL, grp.handle, r, world, tiles, pitch)
            try:
                t.set_points(parts[r])
                t.run()
                labels, kept = t.point_labels()
                ref = reference_ids(parts[r], labels)
                dev = torch.from_numpy(ref).to("cuda:0")
                got = t.compare_labels(dev)
                rows, wall = [], []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    got = t.compare_labels(dev)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    rows.append(t.compare_times())
                down = []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    labels, _ = t.point_labels()
                    down.append((time.perf_counter() - t0) * 1e3)
                keep[r] = (labels, ref, got)
                out[r] = dict(rank=r, kept=kept, points=int(parts[r].shape[0]), annotated=int((ref >= 0).sum()),
                              ms={k: float(np.median([x[k] for x in rows])) for k in tn.C_NAMES}, call_with_download_ms=float(np.median(wall)),
                              point_labels_ms=float(np.median(down)), **t.compare_payload())
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
    res = dict(layout=f"{tiles[0]}x{tiles[1]}", points_per_rank=n_per, repeats=repeats, ranks=out)
    if all(k is not None for k in keep):
        labels, ref = np.concatenate([k[0] for k in keep]), np.concatenate([k[1] for k in keep])
        kept = out[0]["kept"]
        host = []
        for _ in range(min(repeats, 3)):
            t0 = time.perf_counter()
            want = R.compare_labels(labels, ref, kept)
            host.append((time.perf_counter() - t0) * 1e3)
        s = want["summary"]
        res["host_path"] = dict(compare_labels_ms=float(np.median(host)), point_labels_ms=max(o["point_labels_ms"] for o in out),
                                label_bytes_gathered=int(8 * labels.size), same_tables=bool(all(R.same(k[2], want) for k in keep)),
                                annotated=int(s[0]), ids=int(s[3]), cells=int(s[4]), segments=int(kept))
    return res


def main():
    n_per = int(sys.argv[1]) if len(sys.argv) > 1 else 2_500_000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    layouts = sys.argv[3] if len(sys.argv) > 3 else "2x2,4x2"
    for lay in layouts.split(","):
        tx, ty = (int(x) for x in lay.split("x"))
        print(json.dumps(run_layout((tx, ty), n_per, repeats)), flush=True)


if __name__ == "__main__":
    main()
