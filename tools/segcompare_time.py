#!/usr/bin/env python3
"""Time the label comparison (Engine.compare_labels: csrc/segcompare.hip) on URB10M with VGS (config 3, the benchmark scene), next to what
a caller does today: point_labels() to the host and the np.unique path of tests/helpers.py:p2_protocol over N keys.
The reference labelling is made from the engine's own labels and the points: the segment's label where the point sits in an even 4 m
column of the ground plan, a per-column id elsewhere, one point in 50 without annotation -- segments split and merged the way an instance
annotation disagrees with a segmentation, a few hundred ids.
Times are wall-clock around calls that end in a stream synchronisation, medians of repeated warm calls (the first call of each kind
allocates and loads code objects and is not counted):
  compare_device_ms   Engine.compare_labels on a tensor already on the device, the download of the three tables included
  compare_call_ms     vgs_compare_labels_device alone (sizes and summary; the tables stay in HBM)
  host_labels_ms      point_labels(): the N labels to the host
  host_unique_ms      np.unique(label * G + id, return_counts) over the annotated points, and the two arg-max folds over the cells
Prints one JSON line.
Per-kernel split: run the tool with --compares-only under `rocprofv3 --kernel-trace --output-format csv` (a run of its own), then
`tools/segcompare_time.py --split <kernel_trace.csv>` sums the kernels between k_cmp_scan and the last kernel of every compare but the first.
usage: tools/segcompare_time.py [points] [repeats] [--compares-only] | --split <kernel_trace.csv>"""
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def split(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    starts = [i for i, r in enumerate(rows) if r["Kernel_Name"].startswith("k_cmp_scan")]
    per, spans = {}, []
    for a, b in zip(starts[1:], starts[2:] + [len(rows)]):      # every compare but the first
        last = max(i for i in range(a, b) if rows[i]["Kernel_Name"].startswith("k_cmp_"))
        for r in rows[a:last + 1]:
            full = r["Kernel_Name"]
            lib = re.search(r"rocprim::(?:ROCPRIM_\w+::)?(?:detail::)?(\w+)", full)
            own = re.search(r"k_cmp_\w+", full)
            name = own.group(0) if own else ("rocprim " + lib.group(1) if lib else full.split("(")[0].split("<")[0])
            per.setdefault(name, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        spans.append(int(rows[last]["End_Timestamp"]) - int(rows[a]["Start_Timestamp"]))
    n = max(len(spans), 1)
    table = {k: round(sum(v) / n / 1e3, 1) for k, v in sorted(per.items(), key=lambda kv: -sum(kv[1]))}
    print(json.dumps(dict(compares=len(spans), kernel_us_per_compare=table, kernels_us_total=round(sum(table.values()), 1),
                          first_to_last_kernel_us_median=float(np.median(spans)) / 1e3 if spans else None)))


def _median_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def _host_path(eng, ref):
    """what tests/helpers.py:p2_protocol does with two label arrays: the cells by np.unique over the points, then the best overlaps"""
    t = time.perf_counter()
    lab = eng.point_labels()
    t_labels = time.perf_counter() - t
    t = time.perf_counter()
    ok = ref >= 0
    lt, lr = lab[ok].astype(np.int64) + 1, ref[ok].astype(np.int64)
    nt = int(lt.max(initial=0)) + 1
    uk, cnt = np.unique(lr * nt + lt, return_counts=True)
    best_ref = np.zeros(int(lr.max(initial=0)) + 1, np.int64)
    np.maximum.at(best_ref, uk // nt, cnt)
    best_seg = np.zeros(nt, np.int64)
    np.maximum.at(best_seg, uk % nt, cnt)
    return t_labels * 1e3, (time.perf_counter() - t) * 1e3, uk.size


def main():
    import torch

    import vgs_svgs_segmentation_amd as v
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if len(args) > 0 else 10_000_000
    reps = int(args[1]) if len(args) > 1 else 10
    xyz = v.scenes.urban_scene(n)
    eng = v.Engine(v.default_params(2, voxel_size=0.1))
    eng.set_points(xyz)
    eng.run()
    lab = eng.point_labels()
    col = (np.floor(xyz[:, 0] / 4.0).astype(np.int64) & 0x3ff) << 10 | (np.floor(xyz[:, 1] / 4.0).astype(np.int64) & 0x3ff)
    ref = np.where((col & 1) == 0, lab.astype(np.int64), (1 << 20) + col)
    ref[::50] = -1
    ref = ref.astype(np.int32)
    dev = torch.from_numpy(ref).to("cuda:0")
    torch.cuda.synchronize()
    sizes = (C.c_int64(0), C.c_int64(0))
    summary = np.zeros(12, np.int64)

    def call():
        eng._ck(eng._L.vgs_compare_labels_device(eng._h, C.c_void_p(dev.data_ptr()), n, C.byref(sizes[0]), C.byref(sizes[1]),
                                                 summary.ctypes.data_as(C.c_void_p)))

    if "--compares-only" in sys.argv:
        for _ in range(reps + 1):
            call()
        return
    full, full_min = _median_ms(lambda: eng.compare_labels(dev), reps)
    raw, raw_min = _median_ms(call, reps)
    host = [_host_path(eng, ref) for _ in range(min(reps, 3) + 1)][1:]
    c = eng.counts()
    print(json.dumps(dict(points=int(n), segments=c["kept"], annotated=int(summary[0]), cells=sizes[0].value, ids=sizes[1].value, repeats=reps,
                          compare_device_ms=full, compare_device_ms_min=full_min, compare_call_ms=raw, compare_call_ms_min=raw_min,
                          host_labels_ms=float(np.median([h[0] for h in host])), host_unique_ms=float(np.median([h[1] for h in host])),
                          host_cells=int(host[0][2]), host_calls=len(host))), flush=True)
    eng.close()


if __name__ == "__main__":
    if "--split" in sys.argv:
        split(sys.argv[sys.argv.index("--split") + 1])
    else:
        main()
