#!/usr/bin/env python3
"""Time the connected parts of a per-point labelling of the tiled driver (NativeTiles.label_components:
vgs_tiles_point_label_components) on scenes.tiled_urban_scene, ranks as threads of one process over LocalGroup on one GPU.  The labellings
are the rank's refined labels (refine_labels() once, untimed) and one label for every point, torch tensors on the device, read in place.
Per layout and rank: the wall time of the (always collective) call split into the phases of vgs_tiles_get_point_label_component_times --
own parts on the rank's GPU, exchange 1, the link step on its GPU, exchange 2, the host fold, the part ids on its GPU -- and the rank's
payload (vgs_tiles_get_point_label_component_payload: band records, local parts, link triples, bytes put into the two all-gathers).  Beside
them, as the yardstick, one plain Engine's label_components on the gathered points with the gathered labels (the single-context call).
The stages run once, untimed.  The median over the repeats after one warm-up call is printed, one JSON line per layout.
usage: tools/tiles_labelcc_time.py [points per rank] [repeats] [layouts, e.g. 2x2,4x2]"""
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
    fine_of = [None] * world

    def rank_main(r):
        try:
            t = tn.NativeTiles(v.default_params(2, voxel_size=0.1), tn.COMM_LOCAL, grp.handle, r, world, tiles, pitch)
            try:
                n = parts[r].shape[0]
                t.set_points(parts[r])
                t.run()
                _, kept = t.point_labels()
                t.refine_labels()
                fine_of[r] = t.refined_labels().copy()
                fine = torch.from_numpy(fine_of[r]).to("cuda:0")
                one = torch.zeros(n, dtype=torch.int32, device="cuda:0")
                res = dict(rank=r, kept=kept, points=int(n))
                res["refined"] = _timed(repeats, lambda: t.label_components(fine, kept), t.label_component_times, t.label_component_payload)
                res["refined_parts"] = t.label_components(fine, kept)["n_parts"]
                res["one_label"] = _timed(repeats, lambda: t.label_components(one, 1), t.label_component_times, t.label_component_payload)
                res["one_label_parts"] = t.label_components(one, 1)["n_parts"]
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
    res = dict(layout=f"{tiles[0]}x{tiles[1]}", points_per_rank=n_per, repeats=repeats, ranks=out)
    if all(f is not None for f in fine_of):
        # the yardstick: one context over the gathered points
        eng = v.Engine(v.default_params(2, voxel_size=0.1))
        eng.set_points(np.concatenate(parts))
        eng.run()
        kept = out[0]["kept"]
        fine = torch.from_numpy(np.concatenate(fine_of)).to("cuda:0")
        one = torch.zeros(fine.shape[0], dtype=torch.int32, device="cuda:0")
        single = {}
        for name, lab, K in (("refined", fine, kept), ("one_label", one, 1)):
            eng.label_components(lab, K)
            wall = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                c = eng.label_components(lab, K)
                wall.append((time.perf_counter() - t0) * 1e3)
            single[name] = dict(call_ms=float(np.median(wall)), n_parts=c["n_parts"])
        res["single_context"] = single
    return res


def main():
    n_per = int(sys.argv[1]) if len(sys.argv) > 1 else 2_500_000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    layouts = sys.argv[3] if len(sys.argv) > 3 else "2x2"
    for lay in layouts.split(","):
        tx, ty = (int(x) for x in lay.split("x"))
        print(json.dumps(run_layout((tx, ty), n_per, repeats)), flush=True)


if __name__ == "__main__":
    main()
