"""Seeded scenes that drive the supervoxel stage (csrc/vccs.hip) and the SVGS node graph (csrc/svgs.hip) to the paths that street-like
scenes do not reach, and the predicates -- plain numpy over a voxel table -- that say which path a scene reaches.
tests/test_supervoxel_scenes_cpu.py proves every scene's path with the CPU oracle alone; tests/test_gpu_supervoxel_limits.py runs the
engine on them.  Generated, never stored.  This module does not import the engine.

A voxel table is the dict of oracle.voxelize(xyz, res).voxel_table() (vccs_mode 0: the class's own octree, grown from the first point)
or of oracle.voxelize(xyz, res, bbox_first=True).voxel_table() (vccs_mode 1: the adjacency octree's own lattice); its voxels stand in
descending Morton order (the octree's leaf order), so an aligned 8 x 8 x 8 block of lattice cells -- a TILE, key >> 3 -- is one run of the table.

The figures in the docstrings are what the oracle gives on these builders (tests/test_supervoxel_scenes_cpu.py asserts the bound each
one stands for): m0 / m1 = vccs_mode 0 / 1."""
import numpy as np

SUPERVOXEL_DEFAULTS = dict(voxel_size=0.1, seed_size=0.25, graph_size=0.5)


# ---------------------------------------------------------------- builders for svgs_supervoxels
def lattice_cloud(shape, res, origin, seed, jitter=0.2):
    """One point per cell of a shape[0] x shape[1] x shape[2] lattice of pitch `res` whose lower corner is `origin`: the cell's centre
    plus a uniform jitter of +-`jitter` cells per axis, then permuted (seeded)."""
    rng = np.random.default_rng(seed)
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    pts = np.asarray(origin, dtype=np.float64) + (idx + 0.5 + rng.uniform(-jitter, jitter, idx.shape)) * res
    return pts[rng.permutation(pts.shape[0])].astype(np.float32)


def block_1p1():
    """A solid block of 16^3 voxels of 0.1 m, seed_size 0.11: (int)(1.8f * seed / voxel) = 1.
    m1: no expansion round at all, the labels are the kept seeds (3 110 seeds, one voxel each of 4 096).  m0: one round, 2 398
    supervoxels.  labels_per_tile 293 (m0) / 468 (m1) > 32; labels_per_256 232 (m0) / 239 (m1) > 128; labels_per_27 24 (m0) / 27 (m1) >= 6."""
    return lattice_cloud((16, 16, 16), 0.1, (0.3, 0.2, 0.1), seed=101), dict(SUPERVOXEL_DEFAULTS, seed_size=0.11)


def block_1p5():
    """The block of block_1p1 with seed_size 0.15: (int)(1.8f * 1.5) = 2, one round in m1 and two in m0.
    labels_per_tile 185 (m0) / 59 (m1) > 32; labels_per_27 19 (m0) / 9 (m1) >= 6; m1: 1 331 seeds, max_label 1 312, 191 supervoxels
    left at the end, 4.9 % of the voxels without a label."""
    return lattice_cloud((16, 16, 16), 0.1, (0.3, 0.2, 0.1), seed=101), dict(SUPERVOXEL_DEFAULTS, seed_size=0.15)


def block_2p5_origin():
    """A solid block of 18 x 16 x 14 voxels of 0.1 m centred on (0, 0, 0), seed_size 0.25 (a block of 16^3 fills m1's lattice, which is
    centred on the cloud, with eight equal tiles of 729 entries: 18 voxels along x make it 32 wide, with a layer one voxel thick in the
    outer tiles).  tile_entries m1: 16 tiles, own + shell = 448 + 272 = 720 > 448 in the eight inner ones and 56 + 88 = 144 <= 448 in
    the eight thin ones -- k_pclt_normals takes both of its forms in one run; own voxels up to 448 (m1) / 348 (m0) > 64 and shells up to
    272 (m1) / 342 (m0) > 128.  The normals' flip towards the viewpoint (0, 0, 0) changes sign inside the cloud: the coordinates have
    both signs on every axis."""
    return lattice_cloud((18, 16, 14), 0.1, (-0.9, -0.8, -0.7), seed=102), dict(SUPERVOXEL_DEFAULTS)


def line_3000():
    """3000 x 1 x 1 voxels of 0.1 m along x, seed_size 0.25: a chain of about 1 200 supervoxels (m0: 1 201; m1: 1 201 seeds kept, max_label
    1 200, 938 left at the end) whose labels rise along the line (the order of the seed cells is the order along x); a tile holds at most
    9 (m0) / 6 (m1) voxels of its own and 11 / 10 entries; labels_per_256 129 (m0) / 200 (m1)."""
    return lattice_cloud((3000, 1, 1), 0.1, (0.0, 0.0, 0.0), seed=103), dict(SUPERVOXEL_DEFAULTS)


def big_voxels():
    """16 x 16 x 2 cells of 5 m from (-40, -40, 0), voxel_size 5, seed_size 12.5; graph_size is scaled to 25 for the end-to-end run.  A
    tile is 40 m wide: tile_span 39.5 m (m0) / 36.3 m (m1) >= 32 m = 2^21 fixed-point units on voxels that end with a label."""
    return lattice_cloud((16, 16, 2), 5.0, (-40.0, -40.0, 0.0), seed=104), dict(voxel_size=5.0, seed_size=12.5, graph_size=25.0)


def _clutter(seed=105):
    return np.random.default_rng(seed).uniform(0.0, 20.0, (400, 3))


def all_rejected():
    """400 uniform points in a cube of 20 m, voxel_size 0.1, seed_size 1.0: a seed needs more than 0.05 * pi * 5^2 = 3.9 voxels within
    0.5 m.  m1: every seed is rejected -- max_label 0, every label 0.  m0 (no rejection): 392 supervoxels."""
    return _clutter().astype(np.float32), dict(SUPERVOXEL_DEFAULTS, seed_size=1.0)


def clutter_and_sheet():
    """all_rejected's points and a sheet of 30 x 30 x 1 voxels at (8, 8, 10).  m1: the clutter's seeds are rejected, the sheet's kept --
    16 supervoxels, 30.7 % of the points without a label; the clutter points that get one lie within a seed_size of the sheet."""
    sheet = lattice_cloud((30, 30, 1), 0.1, (8.0, 8.0, 10.0), seed=106).astype(np.float64)
    pts = np.concatenate([_clutter(), sheet])
    return pts[np.random.default_rng(107).permutation(pts.shape[0])].astype(np.float32), dict(SUPERVOXEL_DEFAULTS, seed_size=1.0)


TINY = {
    "one_point": ([(0.31, 0.42, 0.53)], 1),
    "two_coincident": ([(0.31, 0.42, 0.53), (0.31, 0.42, 0.53)], 1),
    "two_adjacent": ([(0.31, 0.42, 0.53), (0.41, 0.42, 0.53)], 2),
    "two_apart": ([(0.31, 0.42, 0.53), (8.31, 0.42, 0.53)], 2),
}


def tiny(name):
    """Clouds of one and two points (voxel_size 0.1, seed_size 0.5): TINY[name] = (points, the number of voxels they make)."""
    return np.array(TINY[name][0], dtype=np.float32), dict(SUPERVOXEL_DEFAULTS, seed_size=0.5)


SUPERVOXEL_SCENES = dict(block_1p1=block_1p1, block_1p5=block_1p5, block_2p5_origin=block_2p5_origin, line_3000=line_3000,
                         big_voxels=big_voxels, all_rejected=all_rejected, clutter_and_sheet=clutter_and_sheet,
                         **{"tiny_" + k: (lambda k=k: tiny(k)) for k in TINY})
# the scenes that also run end to end (block_1p1 and block_1p5 do not: their supervoxels sit closer than graph_size / 5, and the oracle
# alone needs 7 to 13 s on them)
END_TO_END = ("block_2p5_origin", "line_3000", "big_voxels", "clutter_and_sheet", "all_rejected") + tuple("tiny_" + k for k in TINY)


# ---------------------------------------------------------------- predicates over a voxel table
def voxel_labels(table, point_labels):
    """The supervoxel label of every voxel (0: none) from the labels of its points; asserts that the points of a voxel share one."""
    pv = np.asarray(table["point_voxel"])
    ok = pv >= 0
    lab = np.asarray(point_labels)
    assert (lab[~ok] == 0).all()
    V = np.asarray(table["key"]).shape[0]
    vlab = np.zeros(V, dtype=np.int64)
    vlab[pv[ok]] = lab[ok]
    assert np.array_equal(vlab[pv[ok]], lab[ok]), "the points of a voxel carry different labels"
    return vlab


def morton(key):
    """Morton code of integer keys (n, 3): x in bit 2, y in bit 1, z in bit 0 of every triple (vm_morton)."""
    k = np.asarray(key).astype(np.uint64)
    code = np.zeros(k.shape[0], dtype=np.uint64)
    for b in range(21):
        for a, shift in ((0, 2), (1, 1), (2, 0)):
            code |= ((k[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + shift)
    return code


def _morton_ok(key):
    """The table stands in descending Morton order of its keys (what makes a tile one run)."""
    code = morton(key)
    return bool((code[1:] < code[:-1]).all())


def _tile_ids(key):
    """Tile number of every voxel (runs of equal key >> 3 in table order) and the number of tiles."""
    assert _morton_ok(key)
    t = np.asarray(key).astype(np.int64) >> 3
    head = np.ones(t.shape[0], dtype=bool)
    head[1:] = (t[1:] != t[:-1]).any(axis=1)
    tid = np.cumsum(head) - 1
    assert np.unique(t, axis=0).shape[0] == int(head.sum())   # a tile is ONE run
    return tid, int(head.sum())


def _distinct_per_group(group, lab):
    """Number of distinct labels > 0 in every group (group ids 0 .. G-1)."""
    G = int(group.max(initial=-1)) + 1
    m = lab > 0
    pairs = np.unique(np.stack([group[m], lab[m]], axis=1), axis=0)
    return np.bincount(pairs[:, 0], minlength=G)


def labels_per_tile(table, vlab):
    """Distinct labels among the voxels of every tile: above VT_SLOTS = 32 the per-tile LDS table of k_vccs_expand_tiles and
    k_pclt_sweep<true> is full and contributions go to memory."""
    tid, _ = _tile_ids(table["key"])
    return _distinct_per_group(tid, np.asarray(vlab))


def labels_per_256(vlab):
    """Distinct labels in every aligned run of 256 consecutive voxels (a workgroup of k_vccs_reseed): above VX_SLOTS = 128 its LDS table
    is full."""
    vlab = np.asarray(vlab)
    return _distinct_per_group(np.arange(vlab.shape[0]) // 256, vlab)


def _lookup(key):
    k = np.asarray(key).astype(np.int64)
    code = (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]
    order = np.argsort(code)
    return code[order], order


def _find(sorted_code, order, q):
    """Voxel at the integer keys q (n, 3), -1 where there is none (keys outside 0 .. 2^21 - 1 included)."""
    inside = ((q >= 0) & (q < (1 << 21))).all(axis=1)
    qc = (q[:, 0] << 42) | (q[:, 1] << 21) | q[:, 2]
    pos = np.clip(np.searchsorted(sorted_code, qc), 0, sorted_code.shape[0] - 1)
    hit = inside & (sorted_code[pos] == qc)
    return np.where(hit, order[pos], -1)


def labels_per_27(table, vlab):
    """Distinct labels > 0 in every voxel's 27-neighbourhood, itself included: from 6 on, vccs_best_offer meets a fifth label besides the
    voxel's own and enters its one-at-a-time loop."""
    key = np.asarray(table["key"]).astype(np.int64)
    vlab = np.asarray(vlab)
    sc, order = _lookup(key)
    V = key.shape[0]
    nb = np.zeros((V, 27), dtype=np.int64)
    for o in range(27):
        d = np.array([o % 3 - 1, (o // 3) % 3 - 1, o // 9 - 1])
        u = _find(sc, order, key + d)
        nb[:, o] = np.where(u >= 0, vlab[np.maximum(u, 0)], 0)
    nb.sort(axis=1)
    return ((nb > 0) & np.concatenate([np.ones((V, 1), dtype=bool), nb[:, 1:] != nb[:, :-1]], axis=1)).sum(axis=1)


def tile_entries(table):
    """(own, shell) per tile: its own voxels, and the occupied cells of the one-cell shell around its 8 x 8 x 8 block.  k_pclt_normals
    stages a tile in LDS while own + shell <= VTN_CAP = 448; every tile kernel loops when own > 64 and stages the shell in a third loop
    when shell > 128."""
    key = np.asarray(table["key"]).astype(np.int64)
    tid, T = _tile_ids(key)
    own = np.bincount(tid, minlength=T)
    first = np.concatenate([[0], np.nonzero(np.diff(tid))[0] + 1])
    base = (key[first] >> 3) << 3
    sc, order = _lookup(key)
    g = np.arange(-1, 9)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    cells = cells[((cells < 0) | (cells > 7)).any(axis=1)]
    assert cells.shape[0] == 488
    shell = np.zeros(T, dtype=np.int64)
    for t in range(T):
        shell[t] = int((_find(sc, order, base[t] + cells) >= 0).sum())
    return own, shell


def voxel_centroids(table, xyz):
    """Mean of every voxel's points (float64)."""
    pv = np.asarray(table["point_voxel"])
    ok = pv >= 0
    V = np.asarray(table["key"]).shape[0]
    n = np.bincount(pv[ok], minlength=V)
    x = np.asarray(xyz)[:, :3].astype(np.float64)
    return np.stack([np.bincount(pv[ok], x[ok, a], minlength=V) for a in range(3)], axis=1) / n[:, None]


def tile_span(table, xyz):
    """Per voxel: the largest distance along an axis between its centroid and the centroid of its tile's first voxel.  From 32 m = 2^21
    fixed-point units (1 / 65 536 m) on, k_vccs_expand_tiles and k_pclt_sweep<true> take the `!small` branch."""
    tid, _ = _tile_ids(table["key"])
    first = np.concatenate([[0], np.nonzero(np.diff(tid))[0] + 1])
    cen = voxel_centroids(table, xyz)
    return np.abs(cen - cen[first[tid]]).max(axis=1)


# ---------------------------------------------------------------- scenes for svgs_segment on caller-supplied labels
SV_SIGMA = 0.002   # spread of a supervoxel's four points
HUB_SIZES = (64, 65, 128, 129, 512)   # rows padded to 64, 128, 128, 256 and 512 entries of k_sv_neighbours' sorting network
SV_ROW = 512       # csrc/svgs.hip: entries of a neighbour row


def _sphere(n, radius):
    """n points spread over a sphere (Fibonacci lattice)."""
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def _supervoxels(centres, rng):
    """Four points per centre (sigma = SV_SIGMA), labels 1 .. S in the order of `centres`, points permuted; max_label = S + 1 (the
    supervoxel that carries max_label itself would be dropped)."""
    S = centres.shape[0]
    pts = np.repeat(centres, 4, axis=0) + rng.normal(0.0, SV_SIGMA, (4 * S, 3))
    labels = np.repeat(np.arange(1, S + 1), 4)
    perm = rng.permutation(4 * S)
    return pts[perm].astype(np.float32), labels[perm].astype(np.int32), S + 1


def hub_and_shell(S, graph_size=0.5, centre=(1.0, 2.0, 3.0)):
    """S supervoxels: the hub (label 1) and S - 1 on a sphere of radius 0.92 graph_size around it.  Only the hub sees them all: its row
    holds S entries (itself included, d2 = 0 < r2), every other row far fewer.  Measured largest rows: 64, 65, 128, 129, 512 and 513 for
    S = 64 ... 513; second largest 22, 23, 41, 42, 158 and 158."""
    rng = np.random.default_rng(200 + S)
    centres = np.concatenate([[np.zeros(3)], _sphere(S - 1, 0.92 * graph_size)]) + np.asarray(centre, dtype=np.float64)
    return _supervoxels(centres, rng)


EDGE_HUB = (-4.0, -2.0, -1.0)
EDGE_A = 2.0 ** -9   # half-width of the exact supervoxels: about 2 mm


def hub_edges(graph_size=0.5):
    """A variant of hub_and_shell(129) with a negative centre: the hub (label 1) at EDGE_HUB, 125 noisy supervoxels on the shell, two
    supervoxels made of the same four points (coincident centroids: a tie on d2 in every row that holds both, broken by id), and three
    whose centroids are exact floats at |dx| = one float step below graph_size, graph_size itself and one step above it from the hub's
    exact centroid: the predicate d2 < r2 is strict, so the hub's row holds the first of the three only.  131 supervoxels, labels
    1 .. 131; the hub's row holds 129 entries.
    Returns (xyz, labels, max_label, ids) with ids = dict(hub, twins, inside, on, outside) of 0-based supervoxel ids (label - 1)."""
    rng = np.random.default_rng(329)
    hub = np.asarray(EDGE_HUB, dtype=np.float64)
    shell = _sphere(126, 0.92 * graph_size) + hub

    def noisy(c):
        return c + rng.normal(0.0, SV_SIGMA, (4, 3))

    def exact(c):   # four points placed symmetrically about the float c (tests/test_supervoxel_scenes_cpu.py: the oracle's centroid is c)
        c = np.asarray(c, dtype=np.float32).astype(np.float64)
        return np.array([c + (EDGE_A, 0, 0), c - (EDGE_A, 0, 0), c + (0, EDGE_A, 0), c - (0, EDGE_A, 0)])

    twin = noisy(shell[124])
    x_on = np.float32(hub[0] + graph_size)
    groups = [exact(hub)] + [noisy(c) for c in shell[:124]] + [twin, twin.copy()]
    groups += [exact((np.nextafter(x_on, np.float32(-10.0)), hub[1], hub[2])), exact((x_on, hub[1], hub[2])),
               exact((np.nextafter(x_on, np.float32(10.0)), hub[1], hub[2])), noisy(shell[125])]
    S = len(groups)
    xyz = np.concatenate(groups).astype(np.float32)
    labels = np.repeat(np.arange(1, S + 1), 4).astype(np.int32)
    perm = rng.permutation(labels.shape[0])
    return xyz[perm], labels[perm], S + 1, dict(hub=0, twins=(125, 126), inside=127, on=128, outside=129)


def cloud_40(seed=340):
    """40 supervoxels of four points on a 8 x 5 grid of pitch 0.3 m in the plane z = 1 (labels 1 .. 40 in grid order, max_label 41)."""
    rng = np.random.default_rng(seed)
    gx, gy = (a.ravel() for a in np.meshgrid(np.arange(8) * 0.3, np.arange(5) * 0.3, indexing="ij"))
    return _supervoxels(np.stack([gx + 2.0, gy - 1.0, np.ones_like(gx)], axis=1), rng)


def labellings_40():
    """name -> (xyz, labels, max_label, supervoxels the oracle makes, points left without a supervoxel) on cloud_40."""
    xyz, lab, mx = cloud_40()
    n = lab.shape[0]
    neg = np.where(lab % 3 == 0, -lab, lab)
    return {
        "sparse_ids": (xyz, (lab * 50021).astype(np.int32), 40 * 50021 + 1, 40, 0),
        "every_third_negative": (xyz, neg.astype(np.int32), mx, 27, 52),
        "max_label_20": (xyz, lab, 20, 19, 4 * 21),
        "max_label_1": (xyz, lab, 1, 0, n),
        "max_label_0": (xyz, lab, 0, 0, n),
        "all_zero": (xyz, np.zeros_like(lab), mx, 0, n),
    }


def nan_labelling():
    """cloud_40 with y = NaN in every 17th point, each still carrying its supervoxel's label: (xyz, labels, max_label, bad) with bad =
    the mask of those points.  A non-finite point belongs to no supervoxel, whatever its label (include/vgs.h)."""
    xyz, lab, mx = cloud_40()
    bad = np.arange(lab.shape[0]) % 17 == 0
    xyz = xyz.copy()
    xyz[bad, 1] = np.nan
    return xyz, lab, mx, bad
