"""Seeded scenes that drive the segment tables to their structural limits (tests/test_gpu_segment_limits.py), with the parameters that
make their segmentation known in advance; tests/test_segment_refs_cpu.py confirms those on the CPU oracle.  Generated, never stored.

The knobs follow from the merge rule: a singleton's threshold is vm_cut_threshold(1, cut_thred, 1) = 1 - cut_thred and a pair weight
exp(-D / (2 sig_w^2)) is at most 1, so cut_thred = 0 merges no edge and every used voxel is a segment, while cut_thred = 100 merges every
edge whose weight is not NaN, so every connected group of voxels is one segment.  adjacency_min above any neighbour count leaves
closestCheck without candidates, voxels_min = 0 keeps every cluster, points_min = 0 uses every voxel that holds a point.  A voxel of at
most three points has no covariance and so no valid normal: no acos, no NaN weight, however far from the origin.  The octree's first box
puts the cloud's first point just below a voxel's upper faces, so the controlled scenes start with a point on their voxel lattice."""
import numpy as np

FAR = (3e5, 5e5, 50.0)
# every used voxel its own segment: no weight exceeds 1 - cut_thred = 1
SPLIT = dict(voxel_size=0.1, cut_thred=0.0, points_min=0, voxels_min=0, adjacency_min=1_000_000)
# every connected group of voxels one segment: every weight that is not NaN exceeds 1 - cut_thred = -99
GROUP = dict(voxel_size=0.1, graph_size=0.5, cut_thred=100.0, points_min=0, voxels_min=0, adjacency_min=1_000_000)



def fragmented_plane(side=272, voxel=0.1):
    """side x side voxels of a flat grid at z = 0, twelve points in each on a 4 x 3 lattice 2 cm inside its faces; the first point is the
    upper corner of voxel (0, 0)."""
    i, j = (a.reshape(-1, 1) for a in np.meshgrid(np.arange(side), np.arange(side), indexing="ij"))
    ox, oy = (a.reshape(1, -1) for a in np.meshgrid(np.linspace(0.02, 0.08, 4), np.linspace(0.02, 0.08, 3), indexing="ij"))
    x, y = (i * voxel + ox).reshape(-1), (j * voxel + oy).reshape(-1)
    return np.concatenate([[[voxel, voxel, 0.0]], np.stack([x, y, np.zeros_like(x)], axis=1)]).astype(np.float32)


def wall_on_ground(seed=5, length=150.0, width=3.0, height=2.0, step=0.04):
    """A ground strip and a wall standing along its middle, 3 mm of noise; the first point puts the wall (y = 0) and the ground (z = 0) in
    the middle of a voxel layer."""
    rng = np.random.default_rng(seed)
    x = np.arange(0.0, length, step)
    gx, gy = np.meshgrid(x, np.arange(-width / 2, width / 2, step), indexing="ij")
    ground = np.stack([gx.ravel(), gy.ravel(), rng.normal(0.0, 0.003, gx.size)], axis=1)
    wx, wz = np.meshgrid(x, np.arange(step, height, step), indexing="ij")
    wall = np.stack([wx.ravel(), rng.normal(0.0, 0.003, wx.size), wz.ravel()], axis=1)
    return np.concatenate([[[0.0, -width / 2 - 0.05, -0.05]], ground, wall]).astype(np.float32)


def two_tilted_planes(gap=0.45, step=0.025, side=4.0):
    """z = 0.3 x + 0.2 y on a 2.5 cm lattice, and the same plane `gap` higher."""
    g = np.arange(0.0, side, step)
    gx, gy = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    z = 0.3 * gx + 0.2 * gy
    return np.concatenate([np.stack([gx, gy, z], axis=1), np.stack([gx, gy, z + gap], axis=1)]).astype(np.float32)


BIG_NODES = ([2047], [2048], [2049], [4096], [4097], [10000], [2048, 2048], [1024, 1024, 1024, 1024, 1], [4097, 4097], [2047, 2049],
             [100] * 40 + [47], [4096, 4097, 1807], [3, 2045], [2047, 1, 2048, 1, 2048])


def big_nodes(seed=11, groups=BIG_NODES, voxel=0.1, pitch=3.0):
    """One segment per group: one voxel per entry holding that many points within 1 mm of its centre, the group's voxels side by side
    along x, the groups `pitch` apart along y; the first point, alone at the origin, is a one-point segment of its own."""
    rng = np.random.default_rng(seed)
    pts = [np.zeros((1, 3))]
    for g, sizes in enumerate(groups):
        for i, n in enumerate(sizes):
            c = np.array([(i + 0.5) * voxel, (g + 1) * pitch + 0.5 * voxel, 0.5 * voxel])
            pts.append(c + rng.uniform(-0.001, 0.001, (n, 3)))
    return np.concatenate(pts).astype(np.float32)


Q = 0.25   # point spacing of the degenerate groups: < graph_size, > a voxel's diagonal (one point per voxel), a multiple of the float
           # spacing at 5e5 m, so the shapes stay exact far from the origin
DEGENERATE = {
    "one": [(0, 0, 0)],
    "two": [(0, 0, 0), (Q, 0, 0)],
    "three": [(0, 0, 0), (Q, 0, 0), (0, Q, 0)],
    "line_x": [(k * Q, 0, 0) for k in range(5)],
    "line_xy": [(k * Q, k * Q, 0) for k in range(5)],                               # along (1, 1, 0) / sqrt 2: exact ties
    "plane": [(a * Q, b * Q, 0) for a in range(3) for b in range(3)],
    "cube": [(a * Q, b * Q, c * Q) for a in (0, 1) for b in (0, 1) for c in (0, 1)],  # a triple eigenvalue
    "same": [(Q, Q, Q)] * 7,
}
# +0.0 and -0.0 where the segment's min x, max y and min z lie
SIGNED_ZEROS = [(0.0, -Q, Q), (-0.0, -Q, 0.0), (Q, 0.0, -0.0), (Q, -0.0, 0.0), (0.0, -0.0, Q)]


def degenerate_scene(shift=None):
    """The DEGENERATE groups 2 m apart along x (shifted by `shift`), or without a shift SIGNED_ZEROS first, at the origin.  Returns the
    points and every group's first point index."""
    groups = {} if shift is not None else {"signed_zeros": np.array(SIGNED_ZEROS, dtype=np.float32)}
    for i, (name, g) in enumerate(DEGENERATE.items()):
        p = np.array(g, dtype=np.float64) + [2.0 * (i + 1), 0.0, 0.0]
        groups[name] = (p + np.asarray(shift if shift is not None else (0.0, 0.0, 0.0))).astype(np.float32)
    first, n = {}, 0
    for name, p in groups.items():
        first[name] = n
        n += p.shape[0]
    return np.concatenate(list(groups.values())), first


def thin_segment(seed=21, length=100.0, radius=0.05, step=0.1):
    """A tilted cylinder of 5 cm radius and 100 m length starting at FAR, one point every 10 cm along its axis (at most three in a voxel)."""
    d = np.array([0.6, 0.64, 0.48])
    e1 = np.cross(d, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    rng = np.random.default_rng(seed)
    t = np.arange(0.0, length, step)
    a = rng.uniform(0.0, 2 * np.pi, t.size)
    p = np.asarray(FAR) + t[:, None] * d + radius * (np.cos(a)[:, None] * e1 + np.sin(a)[:, None] * e2)
    return p.astype(np.float32)


