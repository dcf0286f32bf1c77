"""Seeded scenes that drive the merge stage (csrc/merge.hip: crossValidation, closestCheck, union-find, cluster filter, labels) to its
structural limits, with the parameters that make the outcome known in advance and the truth by construction.  Plain numpy, generated and
never stored; tests/test_merge_scenes_cpu.py confirms every claim on the CPU oracle, tests/test_gpu_merge_limits.py runs the engine.

Conventions.  Every scene sits on the exact binary lattice of cut_order_scenes (RES = 0.0625): a point of cell c lies at
(c + 0.5 + offset) * RES: |offset| <= 0.2 in the voxels of one and three points, so at least 0.3 voxel from a face (most sit at the
centre), and <= 0.3 in cut_order_scenes' sheets.  The first point is the anchor, at the upper corner of cells[0]: the octree's first box
is [p - res + eps / 2, p + res - eps / 2), so its faces -- and those of every box it grows into, by whole boxes -- fall on the lattice
and the anchor into cells[0]; it shares that cell and adds no voxel.  Voxel centres are
lattice points, so a squared distance between two voxels is an integer in cells^2: "neighbours" means d^2 < (graph_size / RES)^2 exactly.
In the GROUP scenes (where adjacency alone is the truth) every distance keeps at least 0.2 voxel inside or 0.3 voxel outside graph_size.

Voxel ids are the cells in DESCENDING Morton order of their keys (x most significant).  Keys are the cells plus a constant per axis, so two
rules hold whatever the constants: along a row of fixed y and z ids descend as x ascends, and a cell that is at least as large on every
axis as another has the smaller id.

A scene is a dict: xyz, params (keywords of default_params), cells (C x 3), kinds (points per cell: ONE, FLAT or SHEET), point_cell (cell
index of every point), comp (component id per cell after the merge stage) and the scene's own structure (rows, paths; `size`: voxels of
the cell's component; `clique`: every row is its component).  The closestCheck scenes start with a FLAT cell: the anchor replaces that
voxel's first point, and three points have no normal wherever they lie, while a sheet with a point at its corner would be bent.

  ONE    one point, at the centre unless the scene says otherwise.  Under GROUP (cut_thred = 100, points_min = 0) every voxel is used and
         every local cut returns its whole row.
  FLAT   three points: used with points_min = 2, but at most three points give no covariance, so no valid normal: the voxel weighs exactly
         0.0f against every voxel.  Its local cut returns it alone (0 is not above 1 - cut_thred), and 0.0f >= 0.0f makes every eligible
         target of closestCheck a tie.
  SHEET  twelve points of cut_order_scenes' sheet voxels, normal z: neighbouring sheets connect."""
import numpy as np

import cut_order_scenes as cs
from segment_scenes import GROUP

RES = cs.RES
ONE, FLAT, SHEET = 1, 3, cs.PTS

CLOSEST = dict(voxel_size=RES, graph_size=0.51, points_min=2)      # closestCheck scenes: 8.16 cells, default sigmas and cut_thred
LADDER = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513)
LADDER_ORACLE = tuple(n for n in LADDER if n <= 129)               # what the CPU oracle's n^3 local cuts take in seconds
COUNT_EDGES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
VOXELS_MIN = (0, 3, 4, 7, 8)


def _group(graph_cells, **kw):
    return dict(GROUP, voxel_size=RES, graph_size=graph_cells * RES, **kw)


def _scene(cells, kinds, comp, params, seed, jitter=0.0, **extra):
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    kinds = np.broadcast_to(np.asarray(kinds, dtype=np.int64), cells.shape[:1]).copy()
    assert cells.min() >= 0 and np.unique(cells, axis=0).shape[0] == cells.shape[0]
    rng = np.random.default_rng(seed)
    point_cell = np.repeat(np.arange(cells.shape[0]), kinds)
    k = kinds[point_cell]
    off = np.zeros((point_cell.size, 3))
    off[k == SHEET] = cs._sheet_offsets(rng, int((k == SHEET).sum()))
    off[k == FLAT] = rng.uniform(-0.2, 0.2, (int((k == FLAT).sum()), 3))
    if jitter:
        off[k == ONE] = rng.uniform(-jitter, jitter, (int((k == ONE).sum()), 3))
    xyz = (cells[point_cell] + 0.5 + off) * RES
    anchor = (cells[0] + 1.0) * RES
    if kinds[0] == ONE:       # one more point in cells[0]
        xyz, point_cell = np.concatenate([anchor[None], xyz]), np.concatenate([[0], point_cell])
    else:                     # a FLAT or SHEET voxel keeps its number of points: its first point becomes the anchor
        xyz[0] = anchor
    return dict(xyz=xyz.astype(np.float32), params=params, cells=cells, kinds=kinds, point_cell=point_cell,
                comp=np.asarray(comp, dtype=np.int64), **extra)


# ---------------------------------------------------------------- truth by construction
def cell_voxels(scene, point_voxel):
    """The voxel id of every cell, from a point -> voxel map: every cell one voxel, every voxel one cell."""
    pc, pv = scene["point_cell"], np.asarray(point_voxel)
    C = scene["cells"].shape[0]
    first = np.zeros(C, dtype=np.int64)
    first[pc[::-1]] = np.arange(pc.size)[::-1]
    vox = pv[first].astype(np.int64)
    assert (pv == vox[pc]).all(), "points of one cell in different voxels"
    assert np.array_equal(np.sort(vox), np.arange(C)), "cells and voxels are not one to one"
    return vox


def labels_of_components(comp_v, voxels_min, point_voxel):
    """The merge stage's outputs for a known partition of the voxels: root (smallest id of the component), size of the voxel's component,
    kept label (components above voxels_min numbered by ascending root, else -1), point labels, and the counts clusters / kept."""
    comp_v = np.asarray(comp_v, dtype=np.int64)
    V = comp_v.size
    low = np.full(int(comp_v.max()) + 1, V, dtype=np.int64)
    np.minimum.at(low, comp_v, np.arange(V))
    root = low[comp_v]
    size = np.bincount(root, minlength=V)
    is_root = root == np.arange(V)
    keep = is_root & (size > voxels_min)
    rank = np.cumsum(keep) - keep
    kept = np.where(keep[root], rank[root], -1)
    pv = np.asarray(point_voxel)
    return dict(root=root, size=size[root], kept=kept, point_labels=np.where(pv >= 0, kept[np.maximum(pv, 0)], -1),
                clusters=int(is_root.sum()), n_kept=int(keep.sum()))


def truth(scene, point_voxel):
    """labels_of_components of the scene's own partition, and `vox`, the voxel id of every cell."""
    vox = cell_voxels(scene, point_voxel)
    comp_v = np.empty(vox.size, dtype=np.int64)
    comp_v[vox] = scene["comp"]
    vm = scene["params"].get("voxels_min", 3)
    return dict(labels_of_components(comp_v, vm, point_voxel), vox=vox)


def lattice_adjacency(scene, vox):
    """Every voxel's row by construction: the voxels within graph_size, itself included, by ascending (d^2, id) -- the radius search's
    order.  Integer arithmetic on the cells."""
    cells = scene["cells"]
    r2 = (scene["params"]["graph_size"] / RES) ** 2
    R = int(np.ceil(np.sqrt(r2)))
    C = cells.shape[0]
    order = np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))
    sc = cells[order]
    lo = np.searchsorted(sc[:, 0], sc[:, 0] - R, side="left")
    hi = np.searchsorted(sc[:, 0], sc[:, 0] + R, side="right")
    rows = [None] * C
    for a in range(C):
        cand = np.arange(lo[a], hi[a])
        d = sc[cand] - sc[a]
        d2 = (d * d).sum(axis=1)
        assert (np.abs(d2 - r2) > 1e-3).all()      # no pair sits on the radius
        m = d2 < r2
        ids = vox[order[cand[m]]]
        o = np.lexsort((ids, d2[m]))
        rows[int(vox[order[a]])] = ids[o].tolist()
    return rows


def margins(scene):
    """(largest neighbour distance, smallest non-neighbour distance) in cells, over all pairs within graph_size + 2 cells."""
    cells = scene["cells"]
    g = scene["params"]["graph_size"] / RES
    R = int(np.ceil(g)) + 2
    order = np.argsort(cells[:, 0], kind="stable")
    sc = cells[order]
    hi = np.searchsorted(sc[:, 0], sc[:, 0] + R, side="right")
    near, far = 0.0, np.inf
    for a in range(sc.shape[0]):
        d = sc[a + 1:hi[a]] - sc[a]
        d2 = (d * d).sum(axis=1)
        if (d2 < g * g).any():
            near = max(near, float(np.sqrt(d2[d2 < g * g].max())))
        if (d2 >= g * g).any():
            far = min(far, float(np.sqrt(d2[d2 >= g * g].min())))
    return near, far


# ---------------------------------------------------------------- 1. list capacities of the merge front
def _nearest_cells(n):
    r = np.arange(-5, 6)
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    d2 = (g * g).sum(axis=1)
    sel = np.lexsort((g[:, 2], g[:, 1], g[:, 0], d2))[:n]
    assert d2[sel].max() <= 25
    return g[sel]


def clique_ladder(sizes=LADDER):
    """One clique per size: the n cells nearest a centre, all within 5 cells of it (515 lattice points are), so every pair is at most 10
    cells apart with graph_size 10.24; centres 22 cells apart, so cliques keep 12 cells between them.  Every row of a clique of size n
    has exactly n entries, all connected, all mutual: rows on, just below and just above the 64 positions of k_union_mutual's list and
    the 256 of k_cross's and their multiples, rows that drain the first list in up to nine rounds and the second in up to three.
    `size`: the clique's size per cell.
    The points sit up to 0.2 voxel off their centres and only sig_p and sig_w keep their defaults, so the weights are exp(-d / 1.6) of
    generic centroid distances d <= 0.66, all different: the local cut gives up on a neighbourhood with more than 8192 pair weights
    inside one 2^-22 interval, which 129 voxels of weight 0.0f would be.  Nearest neighbours weigh 0.94 and more and a segment of s
    vertices takes an edge above its last one less 100 / s, so every local cut still returns its whole row."""
    cells, comp = [], []
    for i, n in enumerate(sizes):
        centre = 5 + 22 * np.array([i % 3, (i // 3) % 3, i // 9])
        cells.append(centre + _nearest_cells(n))
        comp += [i] * n
    far = dict(sig_n=1e4, sig_o=1e4, sig_e=1e4, sig_c=1e4)     # the four distances that are 100 without a normal: 0.01 each
    return _scene(np.concatenate(cells), ONE, comp, _group(10.24, **far), 0, jitter=0.2, size=np.asarray(sizes)[comp], clique=True)


BRIDGES = (61, 62, 63)


def bridges(sizes=BRIDGES, base=(32, 8, 8), anchor=(-32, 31, 14)):
    """What the cliques cannot show: a union that k_union_mutual must not lose.  A clique's edges are all redundant and its first hooks
    (every voxel points at its smallest mutual neighbour, k_cross) already join it, so a lost list entry there changes nothing.  Here one
    edge per element joins two parts, no first hook covers it, and it sits at a chosen position of its row's list of mutual entries.
    An element, with t = (X, Y, Z):
      ball   the m cells nearest (X + 14, Y - 3, Z), all within 2.45 cells of it: a clique
      i      (X + 10, Y, Z): 5 cells from the ball's centre, a neighbour of every ball cell and of t
      t      10 cells from i and more than 11.5 from every ball cell (graph_size 10.24)
      w      (X, Y + 4, Z): a neighbour of t alone
    Row i holds itself, the ball and, farthest and so last, t: m + 2 entries, all mutual, t at position m + 1 = 62, 63, 64 around the 64
    positions of k_union_mutual's list.  Ids: along x they descend, so i < t and the edge is taken in row i.  cells[0], the anchor's, is
    a voxel of its own, placed so that in the y key w and t lie on either side of a multiple of 32 while the element's x and z keys stay
    inside one block of 32: w's Morton code is the element's largest, w its smallest id, and t's first hook goes to w, not to i.  The
    component of m + 3 voxels exists only if that one union is made (tests/test_merge_scenes_cpu.py shows from the oracle's lists that
    the first hooks alone leave i and t apart).  Elements lie 32 cells apart along z.
    `bridge`: the cells (i, t, w) per element, `ball`: its cells."""
    cells, comp, bridge, balls = [tuple(np.array(base) + anchor)], [len(sizes)], [], []
    for e, m in enumerate(sizes):
        t = np.array(base) + [0, 0, 32 * e]
        near = _nearest_cells(m)
        assert (near * near).sum(axis=1).max() <= 6
        n0 = len(cells)
        cells += [tuple(t + [0, 4, 0]), tuple(t), tuple(t + [10, 0, 0])] + [tuple(x) for x in (t + [14, -3, 0] + near)]
        bridge.append((n0 + 2, n0 + 1, n0))
        balls.append(n0 + 3 + np.arange(m))
        comp += [e] * (m + 3)
    return _scene(cells, ONE, comp, _group(10.24, sig_n=1e4, sig_o=1e4, sig_e=1e4, sig_c=1e4), 5, jitter=0.2, bridge=bridge, ball=balls,
                  size=np.concatenate([[1], np.repeat([m + 3 for m in sizes], [m + 3 for m in sizes])]))


# ---------------------------------------------------------------- 2. union-find, k_flatten, cluster filter, labels
def snake(rows=70, cols=100):
    """Two serpentines of rows * cols + 2 * (rows - 1) voxels, at z = 5 (the anchor's) and z = 0.  Steps of 3 cells along a row, rows 6
    cells apart, and two connector cells beside each row end ((+2, +2) and (+2, +4): steps of 2.83, 2, 2.83); with graph_size 4 cells only
    consecutive voxels are neighbours (the nearest other pair is 4.47 apart).  Each snake is one component whose graph diameter is its
    length; the two never touch (five cells apart) and their voxel ids interleave: the octree grows downwards from the anchor, a key
    on z is 2^k - 2 in the anchor's layer and 2^k - 7 in the other, which differ in bit 2 first: every 4 x 4 cells change the snake
    (tests/test_merge_scenes_cpu.py counts the changes).  `path`: the cells of each snake in order."""
    xy = []
    for r in range(rows):
        xs = range(cols) if r % 2 == 0 else range(cols - 1, -1, -1)
        xy += [(4 + 3 * i, 6 * r) for i in xs]
        if r < rows - 1:
            xe = 4 + 3 * (cols - 1) + 2 if r % 2 == 0 else 2
            xy += [(xe, 6 * r + 2), (xe, 6 * r + 4)]
    xy = np.array(xy)
    n = xy.shape[0]
    cells = np.concatenate([np.column_stack([xy, np.full(n, z)]) for z in (5, 0)])
    return _scene(cells, ONE, np.repeat([0, 1], n), _group(4.0), 0, path=[np.arange(n), n + np.arange(n)])


def rods(n=2500, voxels_min=0, seed=3, side=40):
    """n rods of 1 .. 8 adjacent cells along x (seeded sizes), one empty cell between the rods of a row, rows two cells apart in y and z,
    inside a cube of `side` cells: with graph_size 1.5 cells a rod is a component (steps of 1 inside, 2 and more between rods).  A block of
    256 consecutive voxel ids is a Morton-contiguous piece of the cube and holds some fifty rods.  `size`: the rod's size per cell."""
    rng = np.random.default_rng(seed)
    cells, comp, sizes = [], [], []
    for z in range(0, side, 2):
        for y in range(0, side, 2):
            x = 0
            while len(sizes) < n:
                L = int(rng.integers(1, 9))
                if x + L > side:
                    break
                cells += [(x + k, y, z) for k in range(L)]
                comp += [len(sizes)] * L
                sizes.append(L)
                x += L + 1
    assert len(sizes) == n and set(sizes) == set(range(1, 9))
    return _scene(cells, ONE, comp, _group(1.5, voxels_min=voxels_min), seed, size=np.asarray(sizes)[comp])


def count_edges(V, kind):
    """Exactly V voxels in slots 3 x 2 x 2 cells apart (graph_size 1.5 cells), slot 0 at the origin: its cell is at most as large as every
    other on every axis, so it is voxel V - 1, the one k_voxel_labels reads the number of kept segments from.
      "singles"      V single cells, voxels_min = 0: every voxel a kept segment, every point's label its voxel id
      "last_single"  single cells and pairs along x, voxels_min = 1, a single at the origin: voxel V - 1 is a dropped root
      "last_pair"    the same with a pair at the origin: voxel V - 1 is the larger id of a kept pair, no root (V >= 2)"""
    assert kind in ("singles", "last_single", "last_pair") and V >= (2 if kind == "last_pair" else 1)
    lens = []
    while sum(lens) < V:
        if kind == "singles":
            want = 1
        elif not lens:
            want = 2 if kind == "last_pair" else 1
        else:
            want = 2 if len(lens) % 2 == 1 else 1
        lens.append(min(want, V - sum(lens)))
    side = 1
    while side ** 3 < len(lens):
        side += 1
    cells, comp = [], []
    for s, L in enumerate(lens):
        base = (3 * (s % side), 2 * ((s // side) % side), 2 * (s // (side * side)))
        cells += [(base[0] + k, base[1], base[2]) for k in range(L)]
        comp += [s] * L
    assert len(cells) == V
    return _scene(cells, ONE, comp, _group(1.5, voxels_min=0 if kind == "singles" else 1), 0, size=np.asarray(lens)[comp], clique=True, last_cell=0)


# ---------------------------------------------------------------- 3. closestCheck's order rules
def _patch(nx, ny, x0, y0, z0):
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return np.stack([gx.ravel() + x0, gy.ravel() + y0, np.full(nx * ny, z0)], axis=1)


def chains(links=40, seed=0):
    """A 6 x 6 patch of parallel sheets and two rows of FLAT voxels three cells apart leading away from it, at y = 2, z = 0: `row_up` towards
    smaller x, voxel ids ascending away from the patch, `row_down` towards larger x, ids descending (both in order away from the patch).  A
    link sees two links on either side (3 and 6 cells; the next is 9 away, graph_size 8.16) and every weight is 0.0f.
      row_up    every link has, at its turn, the links before it (smaller ids, re-attached): the direction rule lets all re-attach, the tie
                rule sends each to the FARTHER of the two (later in scan order) -- the first to the patch.
      row_down  the far end comes first and finds nobody; only the two links within reach of the patch re-attach.
    q7_count_as_index = 0: the count read as an id would hand the far links a patch voxel."""
    P = 3 * links
    up = np.stack([P - 3 * np.arange(1, links + 1), np.full(links, 2), np.zeros(links, dtype=np.int64)], axis=1)
    down = np.stack([P + 5 + 3 * np.arange(1, links + 1), np.full(links, 2), np.zeros(links, dtype=np.int64)], axis=1)
    comp = [0] * (links + 2) + list(range(1, links - 1)) + [0] * 36
    return _scene(np.concatenate([up, down, _patch(6, 6, P, 0, 0)]), [FLAT] * (2 * links) + [SHEET] * 36, comp,
                  dict(CLOSEST, q7_count_as_index=0), seed, row_up=np.arange(links), row_down=links + np.arange(links),
                  patch=2 * links + np.arange(36))


def wide_tie(seed=7):
    """One FLAT voxel two cells above the middle of a 12 x 12 patch of parallel sheets: its row holds more than 64 eligible targets, all
    of weight 0.0f, so every lane of k_cc_pass<true> carries at least one and the cross-lane (w, j) rule decides: the last in scan order.
    q7_count_as_index stays on: the count is the id of a patch voxel, one more tie, at scan position 0."""
    cells = np.concatenate([[[6, 6, 2]], _patch(12, 12, 0, 0, 0)])
    return _scene(cells, [FLAT] + [SHEET] * 144, [0] * 145, dict(CLOSEST, adjacency_min=1), seed, candidate=0, patch=1 + np.arange(144))


CLUMPS = [(s, e) for s in (1, 2, 3, 4) for e in (0, 1, 2, 3, 4)] + [(1, 2), (2, 1), (3, 0), (1, 3), (2, 2)]   # (FLAT voxels, ONE voxels)


def count_as_index(q7, adjacency_min, seed=2):
    """The patch (6 x 6 sheets) at the corner of largest x, y and z: it holds voxel ids 0 .. 35.  25 clumps of 1 .. 4 FLAT voxels in a 2 x 2
    square, 16 cells apart, far from the patch; above a clump, three cells up, 0 .. 4 voxels of one point (unused with points_min = 2)
    within reach of all its voxels.  A clump voxel's row counts n_all = FLAT + ONE voxels of its clump and finds no eligible target in it.
      candidates  n_all + 1 > adjacency_min -- counting used neighbours only would give other sets for adjacency_min 3 and 4
      q7 = 0      nobody re-attaches
      q7 = 1      entry 0 of the scan is n_all read as a voxel id: a patch voxel, 20 cells and more away; every candidate joins the patch
    `n_all`, `n_used`: per cell (0 for the patch)."""
    cells, kinds, n_all, n_used = [], [], [], []
    sq = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)])
    for k, (s, e) in enumerate(CLUMPS):
        base = np.array([16 * (k % 5), 16 * (k // 5), 0])
        cells += [base + sq[:s], base + sq[:e] + [0, 0, 3]]
        kinds += [FLAT] * s + [ONE] * e
        n_all += [s + e] * s + [0] * e
        n_used += [s] * s + [0] * e
    cells = np.concatenate(cells + [_patch(6, 6, 80, 80, 4)])
    kinds, n_all, n_used = np.array(kinds + [SHEET] * 36), np.array(n_all + [0] * 36), np.array(n_used + [0] * 36)
    cand = (kinds == FLAT) & (n_all + 1 > adjacency_min)
    patch = np.flatnonzero(kinds == SHEET)
    comp = 1 + np.arange(cells.shape[0])
    comp[patch] = 0
    if q7:
        comp[cand] = 0
    return _scene(cells, kinds, comp, dict(CLOSEST, q7_count_as_index=q7, adjacency_min=adjacency_min), seed, patch=patch,
                  n_all=n_all, n_used=n_used, candidates=np.flatnonzero(cand),
                  used_only=np.flatnonzero((kinds == FLAT) & (n_used + 1 > adjacency_min)))


def count_as_index_out_of_range(n, seed=4):
    """n = 2 .. 5 FLAT voxels, all mutual neighbours, and nothing else: n_all = n = V, no voxel has that id, the quirk's entry is skipped."""
    assert 2 <= n <= 5
    cells = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1)])[:n]
    return _scene(cells, FLAT, np.arange(n), dict(CLOSEST, q7_count_as_index=1, adjacency_min=1), seed)
