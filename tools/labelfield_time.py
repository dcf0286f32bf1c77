#!/usr/bin/env python3
"""Time the attribute tables of a per-point labelling (csrc/pointfield.hip) on URB10M with VGS (config 3), refinement with fill:
Engine.label_field_stats(refined, field) for 1, 4 and 16 channels and label_class_histogram(refined, classes, 16), labels and attributes
read in place on the device -- beside segment_field_stats / segment_class_histogram over the same tensors on the same engine in the same
session (csrc/segfield.hip sorts V nodes, this pass N points; the node tables describe the voxel labels, so the rows differ where the
refinement moved a point).  Times are wall-clock around a call that ends with a stream synchronisation and the download of the K-row
tables (launches, the sort and its read-back included); nothing is cached, so every repeat does all the work; the first call of each
kind allocates the buffers and is left out.  Prints one JSON line per measurement: the medians and their ratio.
usage: tools/labelfield_time.py [points] [repeats]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vgs_svgs_segmentation_amd as v  # noqa: E402


def _timed(fn, reps):
    """(median ms, min ms, the last result); the first call is not counted"""
    fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        last = fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), last


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    xyz = v.scenes.urban_scene(n)
    eng = v.Engine(v.default_params(2, voxel_size=0.1))
    eng.set_points(xyz)
    eng.run()
    counts = eng.refine_labels()   # (fill is the default)
    c = eng.counts()
    K = c["kept"]
    refined = torch.from_numpy(eng.refined_labels()).to("cuda:0")
    n_lab = int((refined >= 0).sum().item())
    base = dict(config="c3", points=int(n), finite=c["finite"], nodes=c["voxels"], segments=K, labelled=n_lab,
                refined_filled=counts["points_filled"], refined_changed=counts["points_changed"], repeats=reps)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    for ch in (1, 4, 16):
        x = torch.rand((n, ch), generator=gen, device="cuda:0", dtype=torch.float32) * 255.0
        med, mn, got = _timed(lambda: eng.label_field_stats(refined, x), reps)
        nmed, nmn, _ = _timed(lambda: eng.segment_field_stats(x), reps)
        assert int(got["n_valid"][:, 0].sum()) == n_lab - got["n_skipped"]
        print(json.dumps(dict(base, what="label_field_stats", channels=ch, ms_median=med, ms_min=mn, segment_field_stats_ms_median=nmed,
                              segment_field_stats_ms_min=nmn, label_over_segment=med / nmed)), flush=True)
        del x
    n_classes = 16
    cls = torch.randint(0, n_classes, (n,), generator=gen, device="cuda:0", dtype=torch.int32)
    med, mn, got = _timed(lambda: eng.label_class_histogram(refined, cls, n_classes), reps)
    nmed, nmn, _ = _timed(lambda: eng.segment_class_histogram(cls, n_classes), reps)
    assert int(got["hist"].sum() + got["n_outside"].sum()) == n_lab - got["n_skipped"]
    print(json.dumps(dict(base, what="label_class_histogram", classes=n_classes, ms_median=med, ms_min=mn,
                          segment_class_histogram_ms_median=nmed, segment_class_histogram_ms_min=nmn, label_over_segment=med / nmed)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
