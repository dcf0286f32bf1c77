#!/usr/bin/env python3
"""Time the per-segment statistics of caller-supplied point attributes (Engine.segment_field_stats / segment_class_histogram:
csrc/segfield.hip) on URB10M with VGS (config 3): the call with the field already on the device, for 1, 4 and 16 channels, and the class
histogram at 16 classes.  Times are wall-clock around the call, which ends with a stream synchronisation and the download of the K-row
tables (launches, sd_prepare's sort and scans included); nothing is cached, so every repeat does all the work.  bytes_needed is what the
pass must read once -- perm_b and the field rows (or the classes) of the labelled points -- and gbytes_per_s is that over the median time:
an end-to-end rate of the call, not a kernel's share of peak.
Next to each: the obvious torch alternative on the same tensors, with the labels of point_labels_device as index (label -1 sent to a spare
row; that index tensor is made outside the timed window) -- index_add_ of x and x * x into zeroed (K + 1, C) float32 tables, and bincount
of label * n_classes + class.  index_add_ uses float atomics: its low bits change from run to run (`torch_repeatable` reports whether
the first and the last run agreed), which is what the engine's pass is there to avoid.  The same in float64 -- what a variance would
need -- is timed at one channel only, over two calls: it takes seconds per call there (ten million atomic adds to a few hundred rows)
and longer with more channels.  Prints one JSON line per measurement.
usage: tools/segfield_time.py [points] [repeats]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vgs_svgs_segmentation_amd as v  # noqa: E402


class _DevInt32:
    """The engine's label buffer as a torch tensor, without a copy."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr="<i4", data=(ptr, True), version=2)


def _timed(fn, reps, slow_s=8.0):
    """(median ms, min ms, timed calls, the first and the last result).  The first call allocates and loads code objects and is not counted
    -- unless it alone takes more than slow_s seconds: then it is the one sample, and the figure is marked by calls = 1."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    first = last = fn()
    torch.cuda.synchronize()
    warm = (time.perf_counter() - t) * 1e3
    if warm > slow_s * 1e3:
        return warm, warm, 1, first, None
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), reps, first, last


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    xyz = v.scenes.urban_scene(n)
    eng = v.Engine(v.default_params(2, voxel_size=0.1))
    eng.set_points(xyz)
    eng.run()
    c = eng.counts()
    K = c["kept"]
    ptr = eng.point_labels_device_ptr()
    try:
        labels, index = torch.as_tensor(_DevInt32(ptr, n), device="cuda:0"), "point_labels_device"
    except (TypeError, RuntimeError):   # a torch that does not take the array interface: an uploaded copy of the same labels, said in the output
        labels, index = torch.from_numpy(eng.point_labels()).to("cuda:0"), "uploaded copy of point_labels"
    n_lab = int((labels >= 0).sum().item())
    idx = torch.where(labels >= 0, labels, torch.full_like(labels, K)).long()
    base = dict(points=int(n), labelled=n_lab, segments=K, nodes=c["voxels"], repeats=reps, torch_index=index)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    for ch in (1, 4, 16):
        x = torch.rand((n, ch), generator=gen, device="cuda:0", dtype=torch.float32) * 255.0
        med, mn, _, _, _ = _timed(lambda: eng.segment_field_stats(x), reps)
        need = n_lab * (4 + 4 * ch)

        def alt(dt):
            xd = x.to(dt)
            s1 = torch.zeros((K + 1, ch), device=x.device, dtype=dt).index_add_(0, idx, xd)
            s2 = torch.zeros((K + 1, ch), device=x.device, dtype=dt).index_add_(0, idx, xd * xd)
            return s1, s2

        t32, t32min, _, a, b = _timed(lambda: alt(torch.float32), reps)
        out = dict(base, what="field_stats", channels=ch, ms_median=med, ms_min=mn, bytes_needed=need, gbytes_per_s=need / (med * 1e-3) / 1e9,
                   torch_index_add_f32_ms_median=t32, torch_index_add_f32_ms_min=t32min,
                   torch_repeatable=bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])))
        if ch == 1:   # float64 atomics: seconds per call at one channel, and not bounded at more; timed here only, over two calls
            t64, t64min, n64, _, _ = _timed(lambda: alt(torch.float64), min(reps, 2))
            out.update(torch_index_add_f64_ms_median=t64, torch_index_add_f64_ms_min=t64min, torch_index_add_f64_calls=n64)
        print(json.dumps(out), flush=True)
        del x
    n_classes = 16
    cls = torch.randint(0, n_classes, (n,), generator=gen, device="cuda:0", dtype=torch.int32)
    med, mn, _, _, _ = _timed(lambda: eng.segment_class_histogram(cls, n_classes), reps)
    need = n_lab * 8
    tb, tbmin, _, _, _ = _timed(lambda: torch.bincount(idx * n_classes + cls, minlength=(K + 1) * n_classes), reps)
    h = eng.segment_class_histogram(cls, n_classes)["hist"]
    ref = torch.bincount(idx * n_classes + cls, minlength=(K + 1) * n_classes).reshape(K + 1, n_classes)[:K].cpu().numpy()
    print(json.dumps(dict(base, what="class_histogram", classes=n_classes, ms_median=med, ms_min=mn, bytes_needed=need,
                          gbytes_per_s=need / (med * 1e-3) / 1e9, torch_bincount_ms_median=tb, torch_bincount_ms_min=tbmin,
                          equal_to_torch=bool(np.array_equal(h, ref)))), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
