"""numpy float64 restatement of the oriented-box pass (csrc/segbox.hip, include/vgs.h: vgs_get_segment_boxes).

NumPy's elementwise multiply and add are separate IEEE operations (no FMA) and min / max do not depend on the order, so with the
engine's own centroid3 and frame9 the expressions below, in the header's association, reproduce lo3, hi3, half3 and center3 to the bit.
A zero may carry either sign, so callers compare by value (==), without a tolerance."""
import numpy as np


def project(xyz, centroid, frame):
    """t (n, 3) of points xyz (n, 3) about centroid (n, 3) or (3,) in frame (n, 9) or (9,): t_j = (W[0][j] dx + W[1][j] dy) + W[2][j] dz,
    W[r][j] = frame[r*3+j], d = float64(p) - c."""
    d = xyz[:, :3].astype(np.float64) - centroid
    W = np.broadcast_to(frame, (d.shape[0], 9))
    return np.stack([(W[:, 0 + j] * d[:, 0] + W[:, 3 + j] * d[:, 1]) + W[:, 6 + j] * d[:, 2] for j in range(3)], axis=1)


def ref_boxes(xyz, labels, K, centroid3, frame9):
    """The table of K rows over the points labelled 0 .. K-1 (every label must occur): dict of lo3, hi3, half3, center3, frame9."""
    m = labels >= 0
    lab = labels[m].astype(np.int64)
    n = np.bincount(lab, minlength=K)
    assert lab.max(initial=-1) < K and (n > 0).all()
    order = np.argsort(lab, kind="stable")
    lab = lab[order]
    t = project(xyz[m][order], centroid3[lab], frame9[lab])
    starts = np.concatenate([[0], np.cumsum(n)[:-1]])
    lo = np.minimum.reduceat(t, starts, axis=0)
    hi = np.maximum.reduceat(t, starts, axis=0)
    mid = (lo + hi) * 0.5
    W = frame9
    center = np.stack([centroid3[:, r] + ((W[:, 3 * r + 0] * mid[:, 0] + W[:, 3 * r + 1] * mid[:, 1]) + W[:, 3 * r + 2] * mid[:, 2])
                       for r in range(3)], axis=1)
    return dict(lo3=lo, hi3=hi, half3=(hi - lo) * 0.5, center3=center, frame9=frame9)
