#!/usr/bin/env python3
"""Time the connected parts of a per-point labelling (csrc/labelcc.hip) on an urban scene with VGS (voxel_size 0.1; 10 M points is the
benchmark scene, config 3): one vgs_point_label_components_device call over the refined labels, read in place on the device
(vgs_get_refined_labels_device), and over a single-label labelling (every point 0: one giant root) -- and beside each, measured in the
same run on the same input, vgs_point_label_descriptors_device, the pass that shares the sort (csrc/pointseg.hip) and is the yardstick.
Every time is wall-clock around a call that ends with a stream synchronisation (launches and read-backs included; the components' tables
stay in HBM, the descriptors' K rows are copied out); the first call of each kind allocates the buffers and is left out; the medians
and their ratios go to stdout as one JSON line.
Per-kernel split: run the tool with --calls-only refined|single under `rocprofv3 --kernel-trace --output-format csv` (a run of its own),
then `tools/labelcc_time.py --split <kernel_trace.csv>` sums the kernels from k_ps_keys to k_lc_scatter of every call but the first,
grouped as sort (k_ps_*, the radix sort), vertices (heads, scans, lists), rows (the adjacency kernels of the rows built on request), link,
roots (compress, roots) and tables.
usage: tools/labelcc_time.py [points] [repeats] [--calls-only refined|single] | --split <kernel_trace.csv>"""
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GROUPS = (("link", r"k_lc_link"), ("roots", r"k_lc_compress|k_lc_roots"), ("tables", r"k_lc_parts|k_lc_label_first|k_lc_largest|k_lc_scatter"),
          ("vertices", r"k_lc_heads|k_lc_vertices|k_lc_vfirst|k_lc_unused|scan"), ("rows", r"k_adjacency"), ("sort", r"k_ps_|radix|sort|histogram"))


def split(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    starts = [i for i, r in enumerate(rows) if r["Kernel_Name"].startswith("k_ps_keys")]
    per, grp, spans = {}, {}, []
    for a, b in zip(starts[1:], starts[2:] + [len(rows)]):      # every call but the first
        ends = [i for i in range(a, b) if rows[i]["Kernel_Name"].startswith("k_lc_scatter")]
        if not ends:
            continue   # (a call of the yardstick: the descriptor pass starts with k_ps_keys too)
        for r in rows[a:ends[0] + 1]:
            full = r["Kernel_Name"]
            lib = re.search(r"rocprim::(?:ROCPRIM_\w+::)?(?:detail::)?(\w+)", full)
            own = re.search(r"k_(?:lc|ps)_\w+|k_adjacency\w*", full)
            name = own.group(0) if own else ("rocprim " + lib.group(1) if lib else full.split("(")[0].split("<")[0])
            dt = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            per.setdefault(name, []).append(dt)
            g = next((g for g, pat in GROUPS if re.search(pat, name)), "other")
            grp[g] = grp.get(g, 0) + dt
        spans.append(int(rows[ends[0]]["End_Timestamp"]) - int(rows[a]["Start_Timestamp"]))
    n = max(len(spans), 1)
    table = {k: round(sum(v) / n / 1e3, 1) for k, v in sorted(per.items(), key=lambda kv: -sum(kv[1]))}
    print(json.dumps(dict(calls=len(spans), group_us_per_call={k: round(v / n / 1e3, 1) for k, v in sorted(grp.items(), key=lambda kv: -kv[1])},
                          kernel_us_per_call=table, kernels_us_total=round(sum(table.values()), 1),
                          first_to_last_kernel_us_median=float(np.median(spans)) / 1e3 if spans else None)))


def main():
    import torch

    import vgs_svgs_segmentation_amd as v
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    only = sys.argv[sys.argv.index("--calls-only") + 1] if "--calls-only" in sys.argv else None
    if only:
        args.remove(only)
    n = int(args[0]) if len(args) > 0 else 10_000_000
    reps = int(args[1]) if len(args) > 1 else 10
    xyz = v.scenes.urban_scene(n)
    eng = v.Engine(v.default_params(2, voxel_size=0.1))
    eng.set_points(xyz)
    eng.run()
    counts = eng.refine_labels()
    K = eng.counts()["kept"]
    single = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    inputs = {"refined": (eng.refined_labels_device_ptr(), K), "single": (single.data_ptr(), 1)}
    n_parts, skipped = C.c_int64(0), C.c_int64(0)

    def components(ptr, k):
        eng._ck(eng._L.vgs_point_label_components_device(eng._h, C.c_void_p(ptr), n, k, C.byref(n_parts), C.byref(skipped)))

    def describe(ptr, k):
        out = {name: np.zeros((k, w) if w > 1 else k, dtype=dt) for name, dt, w in v.Engine.DESCRIPTOR_FIELDS}
        eng._ck(eng._L.vgs_point_label_descriptors_device(eng._h, C.c_void_p(ptr), n, k, C.byref(skipped),
                                                          *(out[name].ctypes.data_as(C.c_void_p) for name, _, _ in v.Engine.DESCRIPTOR_FIELDS)))

    if only:
        for _ in range(reps + 1):
            components(*inputs[only])
        return
    res = dict(points=int(n), finite=eng.counts()["finite"], nodes=eng.counts()["voxels"], used=eng.counts()["used"], segments=K,
               refined_filled=counts["points_filled"], refined_changed=counts["points_changed"], repeats=reps, step_ms=eng.stage_times()["total"])
    for name, (ptr, k) in inputs.items():
        cc, dd = [], []
        for it in range(reps + 1):
            t = time.perf_counter()
            components(ptr, k)
            t_cc = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            describe(ptr, k)
            t_dd = (time.perf_counter() - t) * 1e3
            if it > 0:   # the first call of each kind allocates the buffers
                cc.append(t_cc); dd.append(t_dd)
        res[name] = dict(labels=int(k), parts=int(n_parts.value), components_ms_median=float(np.median(cc)), components_ms_min=float(np.min(cc)),
                         describe_labels_ms_median=float(np.median(dd)), describe_labels_ms_min=float(np.min(dd)),
                         components_over_describe=float(np.median(cc)) / float(np.median(dd)))
    print(json.dumps(res), flush=True)
    eng.close()


if __name__ == "__main__":
    if "--split" in sys.argv:
        split(sys.argv[sys.argv.index("--split") + 1])
    else:
        main()
