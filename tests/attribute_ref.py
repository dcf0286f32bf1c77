"""Node attributes (csrc/features.hip: centroid, normal, eight eigen features) restated twice for the tests, without any code of the kernel's loop:

* the float32 leg: numpy float32 arithmetic in the order the specification fixes -- sequential sums (np.add.accumulate, which adds element
  by element, never np.sum, which adds pairwise), the mean recomputed as sum / count, the sum of outer products of p - mean (for more
  than three points, else the zero matrix; divided by the count for supervoxels), the eigen solve and the features through the host build
  of csrc/vgs_math.h (oracle.eigen33 / oracle.eigen_features in DevMath mode), the normal flipped towards the viewpoint (0, 0, 1.5) as
  seen from the run's FIRST point.  Equal to the kernel bit for bit or one of the two is wrong.
* the float64 leg: centroid and scatter matrix of the same float points in float64 and np.linalg.eigh, with the project's own criteria
  for the closed-form solver (tests/test_oracle_kat.py::test_eigen33_against_numpy)."""
import numpy as np

F32 = np.float32
VIEW = (F32(0.0), F32(0.0), F32(1.5))     # VS:1394-1396
BRANCHES = ("all_equal", "low_pair", "high_pair", "general")
EPS = F32(1.1920929e-07)                  # VM_EPS_F


def _seq_sum(a):
    """Column sums of a float32 array, one addition after the other starting from +0.0."""
    a = np.concatenate([np.zeros((1,) + a.shape[1:], F32), a.astype(F32)])
    return np.add.accumulate(a, axis=0, dtype=F32)[-1]


def scatter_f32(pts, svgs):
    """(sum, mean, 3 x 3 matrix) of one node's points in run order, in float32."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    cnt = pts.shape[0]
    s = _seq_sum(pts)
    mean = s / F32(cnt)
    C = np.zeros((3, 3), F32)
    if cnt > 3:                                                  # VS:1554
        d = pts - mean
        prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], axis=1)
        u = _seq_sum(prod)
        C = np.array([[u[0], u[1], u[2]], [u[1], u[3], u[4]], [u[2], u[4], u[5]]], F32)
        if svgs:
            C = C / F32(cnt)                                     # SS:1425
    return s, mean, C


def flip(n, first):
    """The normal turned towards VIEW as seen from `first`: negated when (n . (VIEW - first)) < 0, summed from the left."""
    n = np.asarray(n, F32)
    v = [VIEW[a] - F32(first[a]) for a in range(3)]
    dot = (n[0] * v[0] + n[1] * v[1]) + n[2] * v[2]
    return n * F32(-1.0) if dot < 0 else n.copy()


def node_f32(oracle, pts, svgs, first=None):
    """One node's attributes from its points in run order.  first: the point the normal is flipped by (default: the run's first).
    Returns centroid, normal, eigen (8), evals (ascending, as the solver returns them), C (the float32 matrix), branch, roots2."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    _, mean, C = scatter_f32(pts, svgs)
    ev, evec = oracle.eigen33(C, 1)
    n = flip(evec[:, 0], pts[0] if first is None else first)
    branch, roots2 = solver_branch(C, ev)
    return dict(centroid=mean, normal=n, eigen=oracle.eigen_features(ev, bool(svgs), 1), evals=ev, C=C, branch=branch, roots2=roots2)


def solver_branch(C, ev):
    """Which branch of vm_eigen33 a matrix took, from the returned eigenvalues over the matrix's largest entry, by the solver's own
    conditions; and whether the roots came from vm_roots2 (the only path that returns an exact zero as the lowest root)."""
    scale = np.abs(np.asarray(C, F32)).max()
    if scale <= F32(1.17549435e-38):
        scale = F32(1.0)
    e = np.asarray(ev, F32) / scale
    if e[2] - e[0] <= EPS:
        b = "all_equal"
    elif e[1] - e[0] <= EPS:
        b = "low_pair"
    elif e[2] - e[1] <= EPS:
        b = "high_pair"
    else:
        b = "general"
    return b, bool(ev[0] == 0)


def nodes_f32(oracle, xyz, start, point_idx, used, svgs):
    """node_f32 over a voxel (or supervoxel) table; unused nodes keep zeros, as the records do."""
    V = len(start) - 1
    out = dict(centroid=np.zeros((V, 3), F32), normal=np.zeros((V, 3), F32), eigen=np.zeros((V, 8), F32), evals=np.zeros((V, 3), F32),
               C=np.zeros((V, 3, 3), F32), branch=np.full(V, "", dtype=object), roots2=np.zeros(V, bool))
    for v in np.flatnonzero(used):
        r = node_f32(oracle, xyz[point_idx[start[v]:start[v + 1]], :3], svgs)
        for k in out:
            out[k][v] = r[k]
    return out


# ---------------------------------------------------------------- the float64 leg
def node_f64(pts, svgs):
    """(centroid, matrix, eigenvalues ascending, eigenvectors) of the float points in float64; the matrix follows the same rule for at most
    three points (zero) and for supervoxels (divided by the count)."""
    x = np.asarray(pts, F32).reshape(-1, 3).astype(np.float64)
    m = x.mean(axis=0)
    C = np.zeros((3, 3))
    if x.shape[0] > 3:
        d = x - m
        C = d.T @ d
        if svgs:
            C = C / x.shape[0]
    w, v = np.linalg.eigh(C)
    return m, C, w, v


def f64_figures(pts, svgs, centroid, normal, evals):
    """The figures of the float64 leg for one node: each as (value, bound).
      centroid: |m - m64| per axis against cnt * 2^-23 * max |x| of that axis (a sequential float sum of cnt terms and one division);
      evals:    |ev - w| against 3e-4 * lambda_max + 2e-3 * |w|;
      norm:     | |n| - 1 | against 1e-4;
      residual: |C n - ev[0] n| against 5e-3 * lambda_max.
    `evals` are the float32 leg's (the engine does not export them); centroid and normal are the values under test."""
    x = np.asarray(pts, F32).reshape(-1, 3)
    m, C, w, _ = node_f64(x, svgs)
    lmax = np.abs(w).max()
    n = np.asarray(normal, np.float64)
    ev = np.asarray(evals, np.float64)
    return dict(centroid=(np.abs(np.asarray(centroid, np.float64) - m), x.shape[0] * 2.0 ** -23 * np.abs(x.astype(np.float64)).max(axis=0)),
                evals=(np.abs(ev - w), 3e-4 * lmax + 2e-3 * np.abs(w)),
                norm=(abs(np.linalg.norm(n) - 1.0), 1e-4),
                residual=(np.linalg.norm(C @ n - ev[0] * n), 5e-3 * lmax))


def f64_failures(fig):
    """Names of the criteria a node misses.  centroid and evals are closed bounds (assert_allclose's <=); norm and residual are strict as in
    test_eigen33_against_numpy, except that for the zero matrix (lambda_max = 0, bound 0) the residual has to be exactly zero."""
    bad = []
    if not (fig["centroid"][0] <= fig["centroid"][1]).all():
        bad.append("centroid")
    if not (fig["evals"][0] <= fig["evals"][1]).all():
        bad.append("evals")
    if not fig["norm"][0] < fig["norm"][1]:
        bad.append("norm")
    r, b = fig["residual"]
    if not (r < b or (b == 0 and r == 0)):
        bad.append("residual")
    return bad


def f64_leg(xyz, svgs, start, pidx, used, centroid, normal, evals, skip=()):
    """Nodes that miss the float64 leg: [(node, points, {criterion: (value, bound)})]."""
    bad = []
    for v in np.flatnonzero(used):
        if v in skip:
            continue
        fig = f64_figures(xyz[pidx[start[v]:start[v + 1]], :3], svgs, centroid[v], normal[v], evals[v])
        miss = f64_failures(fig)
        if miss:
            bad.append((int(v), int(start[v + 1] - start[v]), {k: fig[k] for k in miss}))
    return bad


def check_features(eigen8, evals, svgs):
    """eigen8 within rtol 1e-5, atol 1e-6 of helpers.ref_features of the eigenvalues where both are finite; NaN in the same places."""
    from helpers import ref_features
    want = ref_features(np.asarray(evals, F32), svgs)
    got = np.asarray(eigen8, F32)
    assert np.array_equal(np.isnan(got), np.isnan(want)), np.flatnonzero((np.isnan(got) != np.isnan(want)).any(axis=1))[:5]
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    fin = np.isfinite(want)
    over = np.abs(got[fin].astype(np.float64) - want[fin]) - (1e-6 + 1e-5 * np.abs(want[fin].astype(np.float64)))
    assert (over <= 0).all(), f"{int((over > 0).sum())} features outside the tolerance, by up to {float(over.max()):.3g}"
