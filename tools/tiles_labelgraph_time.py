#!/usr/bin/env python3
"""Time the adjacency graph of a per-point labelling of the tiled driver (NativeTiles.label_graph: vgs_tiles_point_label_graph) on
scenes.tiled_urban_scene, ranks as threads of one process over LocalGroup on one GPU.  The labellings are the rank's refined labels
(refine_labels() once, untimed) and its own point labels, torch tensors on the device, read in place.  Per layout and rank: the wall time
of the (always collective) call split into the phases of vgs_tiles_get_label_graph_times -- the own pass on the rank's GPU, exchange 1,
the partial table on its GPU, exchange 2, the host fold -- and the rank's payload (vgs_tiles_get_label_graph_payload: band records, other
ranks' records found in its grid, edges of its partial table, bytes put into the two all-gathers).  Beside them, as the yardstick, one
plain Engine's label_graph on the gathered points with the gathered labels (the single-context call), in the same run.
The stages run once, untimed.  The median over the repeats after one warm-up call is printed, one JSON line per layout.
usage: tools/tiles_labelgraph_time.py [points per rank] [repeats] [layouts, e.g. 2x2,4x2]"""
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
    fine_of, own_of = [None] * world, [None] * world

    def rank_main(r):
        try:
            t = tn.NativeTiles(v.default_params(2, voxel_size=0.1), tn.COMM_LOCAL, grp.handle, r, world, tiles, pitch)
            try:
                t.set_points(parts[r])
                t.run()
                pl, kept = t.point_labels()
                own_of[r] = pl.copy()
                t.refine_labels()
                fine_of[r] = t.refined_labels().copy()
                fine = torch.from_numpy(fine_of[r]).to("cuda:0")
                own = torch.from_numpy(own_of[r]).to("cuda:0")
                res = dict(rank=r, kept=kept, points=int(parts[r].shape[0]))
                res["refined"] = _timed(repeats, lambda: t.label_graph(fine, kept), t.label_graph_times, t.label_graph_payload)
                res["refined_edges"] = t.label_graph(fine, kept)["n_edges"]
                res["own_labels"] = _timed(repeats, lambda: t.label_graph(own, kept), t.label_graph_times, t.label_graph_payload)
                res["own_labels_edges"] = t.label_graph(own, kept)["n_edges"]
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
    if all(f is not None for f in fine_of) and all(isinstance(o, dict) for o in out):
        # the yardstick: one context over the gathered points
        eng = v.Engine(v.default_params(2, voxel_size=0.1))
        eng.set_points(np.concatenate(parts))
        eng.run()
        kept = out[0]["kept"]
        single = {}
        for name, labs in (("refined", fine_of), ("own_labels", own_of)):
            lab = torch.from_numpy(np.concatenate(labs)).to("cuda:0")
            eng.label_graph(lab, kept)
            wall = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                g = eng.label_graph(lab, kept)
                wall.append((time.perf_counter() - t0) * 1e3)
            single[name] = dict(call_ms=float(np.median(wall)), n_edges=g["n_edges"], n_pairs=int(g["n_pairs"].sum()), n_shared=int(g["n_shared"].sum()))
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
