"""Seeded scenes for the point-level label refinement (tests/test_gpu_label_refine.py), with the parameters under which each one reaches
the structural case it is named after; generated, never stored.  SPLIT and GROUP are tests/segment_scenes.py's."""
import numpy as np

from label_refine_ref import floor_and_wall
from segment_scenes import FAR, GROUP, SPLIT

WALL = dict(voxel_size=0.25, graph_size=0.6)


def blob(seed=3, n=20_000, sigma=0.3):
    return np.random.default_rng(seed).normal(0.0, sigma, size=(n, 3)).astype(np.float32)


def _voxel_points(rng, ijk, n, voxel=0.1, margin=0.004):
    """n points uniform inside voxel ijk of a lattice through the origin, `margin` inside its faces"""
    return (np.asarray(ijk, dtype=np.float64) + rng.uniform(margin / voxel, 1.0 - margin / voxel, size=(n, 3))) * voxel


def big_boundary_voxel(seed=9, voxel=0.1):
    """Under SPLIT (every used voxel its own segment): a voxel of 5 000 points between two voxels of 300 and 40 -- several batches, batches
    that start inside a node -- an isolated voxel 3 m away whose only candidate is itself, and a point on the lattice's upper corner
    first (tests/segment_scenes.py: the octree's first box)."""
    rng = np.random.default_rng(seed)
    pts = [np.array([[voxel, voxel, voxel]]), _voxel_points(rng, (2, 2, 2), 5000), _voxel_points(rng, (3, 2, 2), 300),
           _voxel_points(rng, (1, 2, 2), 40), _voxel_points(rng, (30, 2, 2), 25)]
    return np.concatenate(pts).astype(np.float32)


# every used voxel a segment, voxels of at most five points unused, every cluster kept
SPLIT5 = dict(SPLIT, points_min=5)
# every connected group a segment, voxels of at most five points unused, groups of at most two voxels dropped
GROUP5 = dict(GROUP, graph_size=0.25, points_min=5, voxels_min=2)


def dropped_beside_kept(seed=13, voxel=0.1):
    """Under GROUP5 (graph_size 0.25: the 26 lattice neighbours and the axis neighbours two steps away): a kept group of four voxels in a
    row along x; three steps above its end a group of two voxels, out of the kept group's reach and dropped by voxels_min, whose rows hold
    unlabelled nodes only (no candidate: its points keep -1); between the two groups two unused voxels of four points, one of which reaches
    the kept group (filled); an unused voxel far away that reaches nothing; NaN and infinite points last.  (A dropped cluster WITH labelled
    neighbours is what the floor-and-wall scene has.)"""
    rng = np.random.default_rng(seed)
    pts = [np.array([[voxel, voxel, voxel]])]
    pts += [_voxel_points(rng, (2 + i, 2, 2), 30) for i in range(4)]        # kept: four voxels
    pts += [_voxel_points(rng, (2 + i, 2, 5), 30) for i in range(2)]        # dropped: two voxels, three steps up (0.3 > graph_size)
    pts += [_voxel_points(rng, (2, 2, 3), 4), _voxel_points(rng, (2, 2, 4), 4)]   # unused, between them
    pts += [_voxel_points(rng, (40, 2, 2), 4)]                              # unused, alone
    bad = np.array([[np.nan, 0.2, 0.2], [0.25, np.inf, 0.25], [0.25, 0.25, -np.inf], [np.nan, np.nan, np.nan]])
    return np.concatenate(pts + [bad]).astype(np.float32)


def mirror_pair(seed=17):
    """Supervoxels handed in as labels: node 0 (label 1) a noisy patch of the plane z = 0 about (-0.3, 0, 0), node 1 (label 2) its mirror
    image in the plane x = 0, point for point, node 2 (label 3) a patch of the plane z = 0.3 about (0, 0, 0.3) -- and, as node 2's last
    point, (0, 0.002, 0.001) on the mirror plane, far from node 2's own patch and equally far from the other two.  Returns the points, the
    labels and max_label."""
    rng = np.random.default_rng(seed)
    a = np.stack([rng.uniform(-0.4, -0.2, 60), rng.uniform(-0.1, 0.1, 60), rng.normal(0.0, 0.003, 60)], axis=1).astype(np.float32)
    b = a * np.array([-1.0, 1.0, 1.0], dtype=np.float32)
    c = np.stack([rng.uniform(-0.1, 0.1, 60), rng.uniform(-0.1, 0.1, 60), 0.3 + rng.normal(0.0, 0.003, 60)], axis=1).astype(np.float32)
    p = np.array([[0.0, 0.002, 0.001]], dtype=np.float32)
    xyz = np.concatenate([a, b, c, p])
    labels = np.concatenate([np.full(60, 1), np.full(60, 2), np.full(61, 3)]).astype(np.int32)
    return xyz, labels, 4


def grid_supervoxels(xyz, cell=0.3):
    """one supervoxel label per occupied cell of a lattice of `cell`: (labels 1 .., max_label)"""
    key = np.floor(np.asarray(xyz, dtype=np.float64) / cell).astype(np.int64)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    return (inv + 1).astype(np.int32), int(inv.max()) + 2
