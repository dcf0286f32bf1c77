"""Numpy float64 restatements of the per-segment attribute tables (include/vgs.h: vgs_segment_field_stats, vgs_segment_class_histogram).
Every product, quotient and sum is one float64 operation in the header's association; the sums S1 and S2 are numpy's, in whatever order
it takes, so the restatement equals the engine to the bit only where those sums are exact (integer-valued fields), and to a derived bound
elsewhere.  tests/test_segment_fields_ref_cpu.py checks both functions against a per-segment brute force."""
import numpy as np


def ref_field_stats(field, labels, K, anchor):
    """field (N,) or (N, C) float32, labels (N,) with -1 = no segment, anchor (K, C) float64 (the engine's own, or any shift).  Returns
    n_valid, mean, var, vmin, vmax as the header defines them, plus S1, S2 (the sums about the anchor) and A1, A2 (the sums of |d| and of
    d * d over the same values: the scales of the summation error bounds)."""
    field = np.asarray(field, dtype=np.float32)
    if field.ndim == 1:
        field = field[:, None]
    labels = np.asarray(labels)
    C = field.shape[1]
    anchor = np.asarray(anchor, dtype=np.float64).reshape(K, C)
    m = labels >= 0
    lab = labels[m].astype(np.int64)
    x = field[m]
    valid = np.isfinite(x)
    d = np.where(valid, x.astype(np.float64) - anchor[lab], 0.0)
    n = np.zeros((K, C), dtype=np.int64)
    S1, S2, A1 = (np.zeros((K, C), dtype=np.float64) for _ in range(3))
    vmin = np.full((K, C), np.inf, dtype=np.float32)
    vmax = np.full((K, C), -np.inf, dtype=np.float32)
    np.add.at(n, lab, valid.astype(np.int64))
    np.add.at(S1, lab, d)
    np.add.at(S2, lab, d * d)
    np.add.at(A1, lab, np.abs(d))
    np.minimum.at(vmin, lab, np.where(valid, x, np.float32(np.inf)))
    np.maximum.at(vmax, lab, np.where(valid, x, np.float32(-np.inf)))
    some = n > 0
    nn = np.where(some, n, 1).astype(np.float64)
    m1 = S1 / nn
    mean = np.where(some, anchor + m1, np.nan)
    var = np.where(some, np.maximum(0.0, S2 / nn - m1 * m1), np.nan)
    vmin = np.where(some, vmin, np.float32(np.nan)).astype(np.float32)
    vmax = np.where(some, vmax, np.float32(np.nan)).astype(np.float32)
    return dict(n_valid=n, mean=mean, var=var, vmin=vmin, vmax=vmax, S1=S1, S2=S2, A1=A1, A2=S2.copy())


def ref_class_hist(classes, labels, K, n_classes):
    """classes (N,) int32, labels (N,) with -1 = no segment.  Returns hist (K, n_classes), n_outside, majority (the lowest class with the
    largest count, -1 when every count is 0) and majority_count."""
    classes = np.asarray(classes).astype(np.int64)
    labels = np.asarray(labels)
    m = labels >= 0
    lab = labels[m].astype(np.int64)
    cls = classes[m]
    inside = (cls >= 0) & (cls < n_classes)
    hist = np.bincount(lab[inside] * n_classes + cls[inside], minlength=K * n_classes).reshape(K, n_classes).astype(np.int64)
    n_outside = np.bincount(lab[~inside], minlength=K).astype(np.int64)
    best = hist.max(axis=1) if K else np.zeros(0, dtype=np.int64)
    majority = np.where(best > 0, hist.argmax(axis=1) if K else 0, -1).astype(np.int32)   # argmax: the lowest index on a tie
    return dict(hist=hist, n_outside=n_outside, majority=majority, majority_count=best.astype(np.int64))
