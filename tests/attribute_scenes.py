"""Seeded clouds that drive the node-attribute kernel (csrc/features.hip, k_features) to its structural limits and the eigen solver of
csrc/vgs_math.h into each of its branches; tests/test_attribute_ref_cpu.py confirms on the CPU oracle that every property listed here
holds, tests/test_gpu_attributes.py runs the engine on them.  Generated, never stored.

k_features gives a workgroup TB consecutive nodes (256 voxels for VGS, 64 supervoxels for SVGS) = one contiguous range of the gathered
points, and streams that range through LDS in tiles of FEAT_TILE points, twice.  What matters to it is where a node's run lies relative
to the tiles of its workgroup: offset = start[v] - start[TB * g].

Every coordinate is a dyadic rational with few bits (a multiple of 2^-12), so sums, means and the stated properties (a zero matrix, a zero
centroid coordinate, equal eigenvalues) are exact in float32.  The voxel lattice has cell k spanning [(k - 1/2) RES, (k + 1/2) RES) on
every axis, so world coordinate 0 and the viewpoint (0, 0, 1.5) are cell centres: the first point of a VGS cloud is the upper corner of
the lowest cell (the octree's first box then has its faces on this lattice, as in test_gpu_voxel_runs._cloud).

The normal is turned towards the viewpoint as seen from the run's first point.  For a point p = (0, 0, 1.5) + d * axis the flip test
n . (view - p) is exactly -d * n[axis], whatever the rest of n: runs that cross a tile edge keep their first point at +d and the points
that open a later tile at -d along their normal axis, so a first point taken from the wrong tile turns the normal round."""
import numpy as np

RES = 0.25
TILE = 2048                   # FEAT_TILE
TB = {2: 256, 3: 64}          # nodes per workgroup, by method
BIG = 3 * TILE + 500
D = 1.0 / 32                  # the special points' distance from the viewpoint


def _shuffle_keeping_runs(rng, pts, node):
    """Scatter the points (grouped by node, each node's in run order) over the cloud so that every node's points keep their order."""
    n = pts.shape[0]
    slot = rng.permutation(n)
    idx = np.lexsort((slot, node))          # by node, slots ascending inside
    out = np.empty_like(pts)
    out[slot[idx]] = pts
    where = np.empty(n, dtype=np.int64)     # block position -> index in the cloud
    where[:] = slot[idx]
    return out, where


def _morton(k):
    k = np.asarray(k, dtype=np.uint64).reshape(-1, 3)
    code = np.zeros(k.shape[0], dtype=np.uint64)
    for b in range(21):
        for a in range(3):                  # bit triple = x << 2 | y << 1 | z
            code |= ((k[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return code


def _unmorton(code):
    code = np.asarray(code, dtype=np.uint64)
    k = np.zeros((code.shape[0], 3), dtype=np.int64)
    for b in range(21):
        for a in range(3):
            k[:, a] |= (((code >> np.uint64(3 * b + 2 - a)) & np.uint64(1)) << np.uint64(b)).astype(np.int64)
    return k


def _tile_openers(offset, cnt):
    """Run positions k >= 1 at which a run of cnt points that starts at `offset` of its workgroup's range opens a new tile."""
    k = np.arange(1, cnt)
    return k[(offset + k) % TILE == 0]


# ---------------------------------------------------------------- runs_vgs
C0 = np.array([-8, -8, -8])             # the lowest cell; keys are cell - C0
VIEW_CELL = np.array([0, 0, 6])         # holds the viewpoint at its centre
FAR_KEY = 32                            # the second point, on the diagonal: the box grows upwards on all axes at once, no key shifts
N_ABOVE, N_BELOW = 260, 400             # voxels before and after the big one (besides the far one and the anchor)


def runs_vgs(seed=31):
    """VGS, points_min 10 (run again with 0): V = 663 voxels = two full workgroups and one of 151; leaf order is descending Morton code
    of cell - C0, so the sizes are assigned by position.  Table: sizes (points per voxel in leaf order), big / edge_start / edge_first_only
    / edge_end (voxel ids), first_alt {voxel: cloud index of the point a wrong-tile first point would be}."""
    rng = np.random.default_rng(seed)
    big_code = int(_morton(VIEW_CELL - C0)[0])
    codes = np.concatenate([[int(_morton([[FAR_KEY] * 3])[0])], np.arange(big_code + N_ABOVE, big_code - N_BELOW - 1, -1), [0]]).astype(np.uint64)
    cells = _unmorton(codes) + C0
    V = codes.shape[0]
    big = 1 + N_ABOVE
    g0 = big // 256 * 256
    assert V > 512 and V % 256 != 0 and big - g0 >= 5 and (cells[1:-1] - C0).max() < FAR_KEY
    # the first voxel after the big one (a few on) whose cell is centred on x = 0: its first point alone in the earlier tile
    first_only = next(v for v in range(big + 3, g0 + 256) if cells[v][0] == 0)
    sizes = rng.integers(5, 24, size=V)
    sizes[0], sizes[-1] = 1, 1                                    # the far point and the anchor
    sizes[[3, 4, 5, 6, 7, 8, 9]] = [1, 2, 3, 4, 10, 11, 12]       # first workgroup
    sizes[[V - 9, V - 8, V - 7, V - 6, V - 5, V - 4, V - 3, V - 2]] = [11, 1, 2, 3, 4, 10, 11, 17]   # last, partial workgroup
    r = g0
    sizes[r], sizes[r + 1] = 12, 11
    edge_end, edge_start = r + 2, r + 3
    sizes[edge_end] = TILE - 23                                   # ends where the second tile begins ...
    sizes[edge_start] = 15                                        # ... and this one starts there
    sizes[edge_start + 1:big] = 14
    sizes[big], sizes[big + 1] = BIG, 13
    off = int(sizes[g0:first_only - 1].sum())
    fill = (TILE - 1 - off) % TILE
    sizes[first_only - 1] = fill if fill >= 11 else fill + TILE
    sizes[first_only] = 13
    start = np.concatenate([[0], np.cumsum(sizes)])

    pts, node, alt_pos = [], [], {}
    for v in range(V):
        n, c = int(sizes[v]), cells[v].astype(np.float64)
        j = rng.integers(-100, 101, size=(n, 3)) / 256.0
        if v == big:
            j[:, 2] = rng.integers(-16, 17, size=n) / 256.0        # a slab about z = 1.5; the specials on the line x = y = 0
            open_ = _tile_openers(int(start[v] - start[g0]), n)
            j[0] = (0, 0, D / RES)
            j[open_] = (0, 0, -D / RES)
            alt_pos[v] = int(start[v] + open_[-1])
        elif v == first_only:
            j[:, 0] = 0                                            # on the plane x = 0, the first two points either side of it
            j[0], j[1] = (D / RES, 0, 0), (-D / RES, 0, 0)
            alt_pos[v] = int(start[v] + 1)
        p = (c + j) * RES
        if v == V - 1:
            p[0] = (C0 + 0.5) * RES                                # the anchor: upper corner of the lowest cell
        if v == 0:
            p[0] = (C0 + FAR_KEY) * RES
        pts.append(p)
        node.append(np.full(n, v))
    pts, node = np.concatenate(pts), np.concatenate(node)
    head = np.array([start[V - 1], start[0]])                      # anchor first, far point second
    rest = np.setdiff1d(np.arange(pts.shape[0]), head)
    shuf, where = _shuffle_keeping_runs(rng, pts[rest], node[rest])
    xyz = np.concatenate([pts[head], shuf]).astype(np.float32)
    index = np.empty(pts.shape[0], dtype=np.int64)
    index[head] = [0, 1]
    index[rest] = where + 2
    assert np.array_equal(xyz.astype(np.float64), np.concatenate([pts[head], shuf]))   # exact in float32
    table = dict(sizes=sizes, big=big, edge_start=edge_start, edge_end=edge_end, edge_first_only=first_only,
                 first_alt={v: int(index[p]) for v, p in alt_pos.items()})
    return dict(xyz=xyz, method=2, params=dict(voxel_size=RES, points_min=10), table=table)


def run_properties(start, used, tb):
    """What a node table holds for k_features with tb nodes per workgroup.  Per node: offset of its run in its workgroup's range."""
    start = np.asarray(start, dtype=np.int64)
    V = start.shape[0] - 1
    cnt = np.diff(start)
    v = np.arange(V)
    off = start[:-1] - start[v // tb * tb]
    inner = np.asarray(used, bool) & (v % tb != 0)
    wg_first = np.arange(0, V, tb)
    wg_pts = start[np.minimum(wg_first + tb, V)] - start[wg_first]
    return dict(V=V, cnt=cnt, off=off, wg_tiles=(wg_pts + TILE - 1) // TILE,
                on_edge=np.flatnonzero(inner & (off % TILE == 0)),
                first_only=np.flatnonzero(inner & (off % TILE == TILE - 1) & (cnt > 1)),
                ends_on_edge=np.flatnonzero(inner & ((off + cnt) % TILE == 0)))


# ---------------------------------------------------------------- runs_svgs
SV_HEAD = [2048, 1, 2047, 2, 2049, 3, 4, 7000, 63, 64, 65]   # sizes of labels 1 .. 11
SV_V = 2 * 64 + 5
SV_EMPTY = 100                                               # a label below max_label without a point
SV_MAX = SV_V + 2                                            # labels 1 .. SV_MAX - 1 less the empty one are kept; SV_MAX has points and is dropped


def runs_svgs(seed=32):
    """SVGS from caller labels: supervoxel s holds the s-th non-empty label of 1 .. max_label - 1, its points in ascending index.
    Table: sizes (per supervoxel), first_alt {supervoxel: cloud index}, extra (label-0 points), dropped (points of max_label)."""
    rng = np.random.default_rng(seed)
    labels_kept = [l for l in range(1, SV_MAX) if l != SV_EMPTY]
    assert len(labels_kept) == SV_V
    sizes = np.concatenate([SV_HEAD, rng.integers(20, 200, size=SV_V - len(SV_HEAD))])
    start = np.concatenate([[0], np.cumsum(sizes)])
    pts, lab, alt_pos = [], [], {}
    for s, l in enumerate(labels_kept):
        n = int(sizes[s])
        gx, gy = s % 12, s // 12
        c = np.array([1.0 + 0.5 * gx, -3.0 + 0.5 * gy, 0.25 * (s % 5)])
        j = np.stack([rng.integers(-150, 151, size=n), rng.integers(-150, 151, size=n), rng.integers(-10, 11, size=n)], axis=1).astype(np.float64)
        a, b = rng.integers(-2, 3, size=2)
        j[:, 2] += (a * j[:, 0] + b * j[:, 1]) / 4.0           # a tilted patch with a little noise
        p = c + j / 1024.0
        open_ = _tile_openers(int(start[s] - start[s // 64 * 64]), n)
        if n == 2049:                                           # a slab about z = 1.5 beside the viewpoint, specials on x = y = 0
            p = np.array([0.0625, 0.03125, 1.5]) + np.stack([j[:, 0], j[:, 1], rng.integers(-10, 11, size=n)], axis=1) / 1024.0
            p[0], p[open_] = (0, 0, 1.5 + D), (0, 0, 1.5 - D)
            alt_pos[s] = int(start[s] + open_[-1])
        if n == 7000:                                           # a slab about x = 0, specials on y = 0, z = 1.5
            p = np.array([0.0, -0.125, 1.625]) + np.stack([rng.integers(-10, 11, size=n), j[:, 0], j[:, 1]], axis=1) / 1024.0
            p[0], p[open_] = (D, 0, 1.5), (-D, 0, 1.5)
            alt_pos[s] = int(start[s] + open_[-1])
        pts.append(p)
        lab.append(np.full(n, l))
    n_kept = int(start[-1])
    n_drop, n_extra = 50, 300
    pts.append(np.array([8.0, 4.0, 1.0]) + rng.integers(-100, 101, size=(n_drop, 3)) / 1024.0)
    lab.append(np.full(n_drop, SV_MAX))
    pts.append(np.array([4.0, 0.0, 0.5]) + rng.integers(-3000, 3001, size=(n_extra, 3)) / 1024.0)   # unassigned points among the others
    lab.append(np.zeros(n_extra, dtype=np.int64))
    pts, lab = np.concatenate(pts), np.concatenate(lab)
    shuf, where = _shuffle_keeping_runs(rng, pts, np.where(lab == 0, 10_000 + np.arange(lab.shape[0]), lab))
    xyz = shuf.astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64), shuf)
    labels = np.empty(lab.shape[0], dtype=np.int32)
    labels[where] = lab
    table = dict(sizes=sizes, first_alt={s: int(where[p]) for s, p in alt_pos.items()}, extra=n_extra, dropped=n_drop, kept_points=n_kept)
    return dict(xyz=xyz, method=3, params=dict(), labels=labels, max_label=SV_MAX, table=table)


# ---------------------------------------------------------------- degenerate
U = 1.0 / 128


def _families(rng):
    g4 = [(a, b) for a in range(-2, 2) for b in range(-2, 2)]
    pm = [(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]
    half = rng.integers(-80, 81, size=(8, 3)) / 1024.0
    half[:, 0] = np.abs(half[:, 0]) + 1 / 1024.0
    patch = rng.integers(-90, 91, size=(16, 3)) / 1024.0
    patch[:, 2] = (patch[:, 0] - 2 * patch[:, 1]) / 4.0 + rng.integers(-6, 7, size=16) / 1024.0
    fam = {
        "same": np.tile([[4 * U, -2 * U, 6 * U]], (8, 1)),                                  # the exact zero matrix
        "line_x": np.array([(2 * k * U, 2 * U, -4 * U) for k in range(-4, 4)]),
        "line_oblique": np.array([(k * U, 2 * k * U, -k * U) for k in range(-4, 4)]),
        "plane_z": np.array([(2 * a * U, 3 * b * U, 4 * U) for a, b in g4]),                # normal (0, 0, +-1): not a valid normal
        "plane_oblique": np.array([(2 * a * U, 3 * b * U, (2 * a + 3 * b) * U) for a, b in g4]),
        "cube": np.array(pm) * 4 * U,                                                       # three equal eigenvalues
        "slab": np.array(pm) * [8 * U, 8 * U, 2 * U],                                       # the two highest equal
        "rod": np.array(pm) * [2 * U, 2 * U, 8 * U],                                        # the two lowest equal
        "mirror_x": np.concatenate([half, half * [-1, 1, 1]]),                              # centroid x exactly the cell centre's: 0 in cell x = 0
        "control_patch": patch,
        "control_blob": rng.integers(-90, 91, size=(16, 3)) / 1024.0,
    }
    return fam


# the branch of vm_eigen33 each family reaches near the origin, and whether its roots come from vm_roots2
NEAR_BRANCH = {"same": ("all_equal", True), "line_x": ("low_pair", True), "line_oblique": ("low_pair", True), "plane_z": ("general", True),
               "plane_oblique": ("general", True), "cube": ("all_equal", False), "slab": ("high_pair", False), "rod": ("low_pair", False),
               "mirror_x": ("general", False), "control_patch": ("general", False), "control_blob": ("general", False)}
DEG_C0 = np.array([-2, -2, -2])
DEG_NEAR = np.array([0, 2, 3])          # mirror_x first, in the cell centred on x = 0; the others along x
DEG_FAR = np.array([596, 596, 8])       # 149 units out


def degenerate(method, seed=33):
    """One node per family and placement, in one cloud for both methods: a voxel of its own (VGS, points_min 4) that is also a supervoxel
    of its own (SVGS labels 1 ..).  Table: rows of dict(name, family, place, first (cloud index of its first point), label, points,
    fp64_skip (None, or the reason the float64 leg leaves the row out))."""
    rng = np.random.default_rng(seed)
    fam = _families(rng)
    order = ["mirror_x"] + [f for f in fam if f != "mirror_x"]
    pts, lab, rows = [((DEG_C0 + 0.5) * RES)[None]], [np.zeros(1, dtype=np.int64)], []
    n = 1
    for place, base in (("near", DEG_NEAR), ("far", DEG_FAR)):
        for i, f in enumerate(order):
            cell = base + [i, 0, 0]
            p = cell * RES + fam[f]
            assert (np.abs(fam[f]) <= RES / 2 - U).all()
            label = len(rows) + 1
            rows.append(dict(name=f"{f}/{place}", family=f, place=place, first=n, label=label, points=p.shape[0], fp64_skip=None))
            pts.append(p)
            lab.append(np.full(p.shape[0], label))
            n += p.shape[0]
    pts = np.concatenate(pts)
    xyz = pts.astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64), pts)
    params = dict(voxel_size=RES, points_min=4, cut_thred=0.9, voxels_min=1) if method == 2 else dict(cut_thred=0.9)
    return dict(xyz=xyz, method=method, params=params, labels=np.concatenate(lab).astype(np.int32), max_label=len(rows) + 1, table=rows)


# ---------------------------------------------------------------- the cases both test modules run
CASES = ["runs_vgs", "runs_vgs_pm0", "runs_svgs", "degenerate_vgs", "degenerate_svgs"]


def build(case):
    sc = {"runs_vgs": runs_vgs, "runs_vgs_pm0": runs_vgs, "runs_svgs": runs_svgs,
          "degenerate_vgs": lambda: degenerate(2), "degenerate_svgs": lambda: degenerate(3)}[case]()
    if case == "runs_vgs_pm0":
        sc["params"] = dict(sc["params"], points_min=0)
    return sc


def row_nodes(sc, point_node):
    """Node of every row of a degenerate table: the voxel of its first point, or the supervoxel of its label."""
    return [int(point_node[r["first"]]) if sc["method"] == 2 else r["label"] - 1 for r in sc["table"]]
