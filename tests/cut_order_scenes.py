"""Clouds of tests/test_gpu_cut_order.py, plain numpy: "sheet voxels" on an exact lattice.  A sheet voxel holds 12 points (points_min is
10) spread +-0.3 voxel in its plane and +-0.02 voxel across it -- never exactly planar: such a voxel gets no normal and every distance to
it becomes 100.  Points sit at (cell + 0.5 + offset) * RES; one anchor point at a lattice corner comes first, so that the octree's faces
fall on the lattice (as tests/test_gpu_voxel_runs._cloud)."""
import numpy as np

RES = 0.0625          # exact in binary
PTS = 12
PARAMS = dict(voxel_size=RES, graph_size=0.51)


def _place(cells, off):
    """Points of the voxels `cells` (one row each) from per-point offsets in voxels; the first point becomes the anchor of the lattice."""
    xyz = (np.repeat(np.asarray(cells, dtype=np.int64), PTS, axis=0) + 0.5 + off) * RES
    xyz[0] = (np.asarray(cells[0]) + 1.0) * RES
    return xyz.astype(np.float32)


def _sheet_offsets(rng, n):
    off = rng.uniform(-0.3, 0.3, (n, 3))
    off[:, 2] = rng.uniform(-0.02, 0.02, n)
    return off


def block(side, seed=0):
    """side x side x side sheet voxels, all sheets parallel to z = const."""
    g = np.arange(side)
    cells = np.stack([a.ravel() for a in np.meshgrid(g, g, g, indexing="ij")], axis=1)
    rng = np.random.default_rng(seed)
    return _place(cells, _sheet_offsets(rng, cells.shape[0] * PTS))


def _rotations(normals):
    """One rotation matrix per row that takes z to the (unit) normal."""
    n = normals / np.linalg.norm(normals, axis=1, keepdims=True)
    h = np.where(np.abs(n[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    u = np.cross(n, h)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(n, u)
    return np.stack([u, v, n], axis=2)      # columns u, v, n


def singletons(seed=0, group=False):
    """6 x 6 x 6 sheet voxels six cells apart (0.375: the six face neighbours lie inside graph_size 0.51, the next ring at 0.53 does not), each
    sheet turned so that its normal makes more than 35 degrees with the normals of the neighbours placed before it.  With the default
    sigmas a pair weighs exp(-D / 8), D >= sqrt((0.375 / 0.2)^2 + (0.61 / 0.2)^2) = 3.6, below 1 - cut_thred = 0.7 (D = 2.85): every local
    cut returns the voxel alone.  group=True adds a 4 x 4 patch of parallel sheets (normal z; they connect with each other) inside the
    lattice, 3.3 cells from the nearest lattice voxels, whose normals keep more than 50 degrees from z: a kept group for closestCheck to
    attach the isolated voxels around it to."""
    rng = np.random.default_rng(seed)
    g = np.arange(6) * 6
    cells = np.stack([a.ravel() for a in np.meshgrid(g, g, g, indexing="ij")], axis=1)
    n = cells.shape[0]
    gx, gy = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    patch = np.stack([gx.ravel() + 13, gy.ravel() + 13, np.full(16, 15)], axis=1)
    z = np.array([0.0, 0.0, 1.0])
    normals = np.zeros((n, 3))
    for i in range(n):
        near = np.flatnonzero(np.linalg.norm((cells[:i] - cells[i]) * RES, axis=1) < 0.5)
        by_patch = group and np.linalg.norm((patch - cells[i]) * RES, axis=1).min() < 0.6
        while True:
            c = rng.standard_normal(3)
            c /= np.linalg.norm(c)
            if by_patch and abs(c @ z) >= np.cos(np.radians(50.0)):
                continue
            if near.size == 0 or np.abs(normals[near] @ c).max() < np.cos(np.radians(35.0)):
                break
        normals[i] = c
    off = _sheet_offsets(rng, n * PTS)
    off = np.einsum("pij,pj->pi", np.repeat(_rotations(normals), PTS, axis=0), off)
    if group:
        cells = np.concatenate([cells, patch])
        off = np.concatenate([off, _sheet_offsets(rng, 16 * PTS)])
    return _place(cells, off)


def mirrored(seed=0):
    """[anchor, P, mirror(P)], mirror: x -> -x.  P: 4 x 6 x 2 parallel sheet voxels in the cells x >= 0; x = 0 is a voxel face, float negation
    is exact and the points of a voxel come in the same order on both sides, so a pair and its mirror image weigh the same to the bit.  The
    anchor (one more point in the cell at the far corner of P) is not mirrored."""
    g = np.meshgrid(np.arange(4), np.arange(6), np.arange(2), indexing="ij")
    cells = np.stack([a.ravel() for a in g], axis=1)
    rng = np.random.default_rng(seed)
    P = ((np.repeat(cells, PTS, axis=0) + 0.5 + _sheet_offsets(rng, cells.shape[0] * PTS)) * RES).astype(np.float32)
    anchor = (np.array([[4.0, 6.0, 2.0]]) * RES).astype(np.float32)     # corner of cell (3, 5, 1)
    return np.concatenate([anchor, P, P * np.array([-1, 1, 1], dtype=np.float32)])


def translates(seed=0, copies=((1, 1, 0), (4, 2, 0)), side=(6, 5, 2)):
    """A small block of parallel sheet voxels in which the voxels at `copies` hold the same points moved by whole voxels.  Every offset is a
    multiple of 2^-10 voxel and every coordinate below 1, so the float32 points of the copies are exact translates of each other."""
    g = np.meshgrid(*[np.arange(s) for s in side], indexing="ij")
    cells = np.stack([a.ravel() for a in g], axis=1)
    rng = np.random.default_rng(seed)
    off = np.round(_sheet_offsets(rng, cells.shape[0] * PTS) * 1024) / 1024
    off[np.abs(off[:, 2]) < 1 / 1024, 2] = 1 / 1024
    off = off.reshape(-1, PTS, 3)
    idx = [int(np.flatnonzero((cells == np.array(c)).all(axis=1))[0]) for c in copies]
    for i in idx[1:]:
        off[i] = off[idx[0]]
    xyz = (np.repeat(cells, PTS, axis=0) + 0.5 + off.reshape(-1, 3)) * RES
    anchor = (np.array([side], dtype=np.float64)) * RES               # corner of the last cell
    return np.concatenate([anchor, xyz]).astype(np.float32), idx
