"""tests/segment_boxes_ref.py (the numpy restatement the GPU box tests compare against) against a slow loop per segment and per point in
Python floats -- IEEE doubles, one operation at a time, the header's association -- so that a bug in the reference cannot hide a bug in
the kernel.  No GPU."""
import numpy as np
import pytest

from segment_boxes_ref import ref_boxes


@pytest.mark.parametrize("seed,shift", [(1, 0.0), (2, 3e5)])
def test_ref_boxes_against_a_loop(seed, shift):
    rng = np.random.default_rng(seed)
    n, K = 300, 7
    xyz = (rng.normal(0.0, 2.0, (n, 3)) + shift).astype(np.float32)
    labels = rng.integers(-1, K - 1, n).astype(np.int32)
    labels[5] = K - 1                      # a label that occurs once
    cen = np.stack([xyz[labels == k].astype(np.float64).mean(axis=0) for k in range(K)])
    Q = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(K)]).reshape(K, 9)
    ref = ref_boxes(xyz, labels, K, cen, Q)
    for k in range(K):
        W = [[float(Q[k, 3 * r + j]) for j in range(3)] for r in range(3)]
        c = [float(a) for a in cen[k]]
        lo, hi = [np.inf] * 3, [-np.inf] * 3
        for p in xyz[labels == k]:
            dx, dy, dz = float(p[0]) - c[0], float(p[1]) - c[1], float(p[2]) - c[2]
            for j in range(3):
                t = (W[0][j] * dx + W[1][j] * dy) + W[2][j] * dz
                lo[j], hi[j] = min(lo[j], t), max(hi[j], t)
        mid = [(lo[j] + hi[j]) * 0.5 for j in range(3)]
        assert ref["lo3"][k].tolist() == lo and ref["hi3"][k].tolist() == hi
        assert ref["half3"][k].tolist() == [(hi[j] - lo[j]) * 0.5 for j in range(3)]
        assert ref["center3"][k].tolist() == [c[r] + ((W[r][0] * mid[0] + W[r][1] * mid[1]) + W[r][2] * mid[2]) for r in range(3)]
    one = int(np.nonzero(labels == K - 1)[0][0])
    assert (labels == K - 1).sum() == 1
    assert (ref["half3"][K - 1] == 0).all() and (ref["center3"][K - 1] == xyz[one].astype(np.float64)).all()
