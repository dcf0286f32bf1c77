"""The voxel table and the point -> voxel map of the voxelize stage (csrc/voxelize.hip: k_run_counts, k_tile_offsets, k_voxel_runs) against a
numpy restatement, on clouds laid out around the structure of those kernels: tiles of TILE sorted keys, one workgroup each, whose run
heads are counted, offset and written in separate launches.

The restatement: a point's voxel key per axis is floor((p - box.min) / voxel_size) in double arithmetic with the engine's own box, its code
the Morton interleave of the three keys (x most significant); voxels are the distinct codes in DESCENDING order (PCL's leaf iterator),
the points of a voxel in ascending index order.  np.unique gives the codes, the first index and the count of every voxel.  Every point of
a scene sits at least 0.3 voxels away from a voxel face, so no rounding can move it into another voxel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 2048          # VR_TILE of csrc/voxelize.hip
RES = 0.25           # exact in binary: the lattice below is exact in float32


def _cloud(cells, seed=0, jitter=0.2):
    """One point per row of `cells` (integer voxel coordinates), inside its cell; the first point anchors the octree's grid on the lattice."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    xyz = (cells + 0.5 + rng.uniform(-jitter, jitter, cells.shape)) * RES
    xyz[0] = (cells[0] + 1.0) * RES    # the first box is [p - res + eps / 2, p + res - eps / 2): its faces fall on the lattice, the point into cells[0]
    return xyz.astype(np.float32)


def _morton(k):
    code = np.zeros(k.shape[0], dtype=np.uint64)
    for b in range(21):
        for a in range(3):   # bit triple = x << 2 | y << 1 | z
            code |= ((k[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return code


def _expected(xyz, box_min):
    finite = np.isfinite(xyz).all(axis=1)
    idx = np.flatnonzero(finite)
    k = np.floor((xyz[idx].astype(np.float64) - box_min) / RES).astype(np.uint64)
    code = _morton(k)
    uniq, first, inverse, counts = np.unique(code, return_index=True, return_inverse=True, return_counts=True)
    V = uniq.size
    order = np.arange(V)[::-1]                      # voxel v holds the v-th LARGEST code
    pt_vox = np.full(xyz.shape[0], -1, dtype=np.int32)
    pt_vox[idx] = (V - 1 - inverse).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(counts[order])]).astype(np.int32)
    point_idx = idx[np.lexsort((idx, pt_vox[idx]))].astype(np.int32)   # by voxel, ascending index inside
    return dict(V=V, nf=idx.size, key=k[first[order]].astype(np.uint32), first=idx[first[order]].astype(np.int32), counts=counts[order],
                start=start, point_idx=point_idx, pt_vox=pt_vox)


def _key_layout(depth, n):
    """What voxelize_sorted_table chooses: 32-bit keys while the valid bit and 3 * depth code bits fit; else 64-bit keys, with the point
    index packed below the code while it fits too."""
    key_bits = 3 * depth + 1
    idx_bits = 1
    while idx_bits < 32 and (1 << idx_bits) < n:
        idx_bits += 1
    if key_bits <= 32:
        return "u32"
    return "u64-packed" if key_bits + idx_bits <= 64 else "u64"


def _check(gpu, xyz, layout):
    eng = gpu.Engine(gpu.default_params(2, voxel_size=RES))
    eng.set_points(xyz)
    eng.voxelize()
    c = eng.counts()
    assert _key_layout(c["depth"], xyz.shape[0]) == layout, c
    exp = _expected(xyz, eng.bbox()[:3])
    assert (c["points"], c["finite"], c["voxels"]) == (xyz.shape[0], exp["nf"], exp["V"])
    t = eng.voxel_table()
    np.testing.assert_array_equal(t["key"], exp["key"])
    np.testing.assert_array_equal(t["start"], exp["start"])
    np.testing.assert_array_equal(np.diff(t["start"]), exp["counts"])
    np.testing.assert_array_equal(t["point_idx"], exp["point_idx"])
    np.testing.assert_array_equal(t["point_idx"][t["start"][:-1]], exp["first"])
    np.testing.assert_array_equal(eng.point_voxel(), exp["pt_vox"])
    return t, exp


def _random_cells(n, n_cells, extent, seed):
    """n points over n_cells distinct cells of a box of `extent` cells a side (z: an eighth of it), in random order."""
    rng = np.random.default_rng(seed)
    flat = rng.choice(extent * extent * max(extent // 8, 1), size=n_cells, replace=False)
    cells = np.stack([flat % extent, (flat // extent) % extent, flat // (extent * extent)], axis=1)
    return cells[rng.integers(0, n_cells, size=n)]


# extents of the three key layouts: up to 1024 voxels across -> depth <= 10 -> 31 + 1 bits; beyond -> 64-bit keys with the index below the code;
# half a million voxels across -> depth 20 or 21 -> no room for the index, the sort carries it as a value
WIDTHS = [("u32", 200), ("u64-packed", 3000), ("u64", 600_000)]


def _spread(cells, extent):
    """Stretch a scene to `extent` cells across without changing which points share a voxel or the order of the voxels along x."""
    cells = np.asarray(cells, dtype=np.int64).copy()
    far = np.array([[extent - 1, 0, 0], [0, extent - 1, 0]])
    return np.concatenate([cells, far])


@pytest.mark.parametrize("layout,extent", WIDTHS)
def test_size_not_a_multiple_of_the_tile(gpu, layout, extent):
    n = 5 * TILE + 777
    cells = _spread(_random_cells(n - 2, 1500, min(extent, 4000), seed=1), extent)
    assert cells.shape[0] % TILE != 0 and cells.shape[0] % 4 != 0
    _check(gpu, _cloud(cells, seed=1), layout)


# (three points need two index bits: beside a code of depth 20 they would still be packed, so the smallest cloud leaves the third layout out)
@pytest.mark.parametrize("layout,extent,n", [(w, e, n) for n in (3, 301) for w, e in WIDTHS if not (n == 3 and w == "u64")])
def test_smaller_than_one_tile(gpu, layout, extent, n):
    cells = _spread(_random_cells(n - 2, max(n // 4, 1), min(extent, 4000), seed=2), extent)
    assert cells.shape[0] < TILE
    _check(gpu, _cloud(cells, seed=2), layout)


@pytest.mark.parametrize("layout,extent", WIDTHS)
def test_one_voxel_spanning_several_tiles(gpu, layout, extent):
    rng = np.random.default_rng(3)
    big = np.tile([[7, 5, 3]], (3 * TILE + 500, 1))                       # one voxel of more than three tiles ...
    cells = np.concatenate([_random_cells(900, 300, min(extent, 4000), seed=3), big])
    cells = _spread(cells[rng.permutation(cells.shape[0])], extent)     # ... somewhere in the middle of the order
    t, exp = _check(gpu, _cloud(cells, seed=3), layout)
    v = int(np.argmax(exp["counts"]))
    assert exp["counts"][v] >= 3 * TILE + 500 and t["start"][v] // TILE + 3 <= (t["start"][v + 1] - 1) // TILE


@pytest.mark.parametrize("layout,extent", WIDTHS)
def test_every_point_in_its_own_voxel(gpu, layout, extent):
    n = 2 * TILE + 1234
    rng = np.random.default_rng(4)
    ext = min(extent, 4000)
    flat = rng.choice(ext * ext, size=n - 2, replace=False)
    flat = flat[(flat != ext - 1) & (flat != (ext - 1) * ext)]   # (the two far cells come with _spread)
    cells = _spread(np.stack([flat % ext, flat // ext, np.zeros_like(flat)], axis=1), extent)
    t, exp = _check(gpu, _cloud(cells, seed=4), layout)
    assert exp["V"] == cells.shape[0] and (exp["counts"] == 1).all()


@pytest.mark.parametrize("layout,extent", WIDTHS)
def test_run_head_exactly_on_a_tile_boundary(gpu, layout, extent):
    """Voxels in descending code order: the far cell on x (one point), then x = 5 with TILE - 1 points, x = 4 with TILE points, x = 3 with 4 points,
    ...: heads at sorted positions TILE and 2 * TILE, the first keys of the second and third workgroup, and at 2 * TILE + 4, the first key of a thread."""
    rng = np.random.default_rng(5)
    groups = [((5, 0, 0), TILE - 1), ((4, 0, 0), TILE), ((3, 0, 0), 4), ((2, 0, 0), 700), ((1, 0, 0), 9)]
    cells = np.concatenate([np.tile([c], (k, 1)) for c, k in groups])
    cells = np.concatenate([cells[rng.permutation(cells.shape[0])], [[extent - 1, 0, 0]]])
    t, exp = _check(gpu, _cloud(cells, seed=5), layout)
    np.testing.assert_array_equal(t["start"], [0, 1, TILE, 2 * TILE, 2 * TILE + 4, 2 * TILE + 704, 2 * TILE + 713])


@pytest.mark.parametrize("layout,extent", WIDTHS)
def test_non_finite_points_sort_to_the_end(gpu, layout, extent):
    n = 3 * TILE + 50
    cells = _spread(_random_cells(n - 2, 800, min(extent, 4000), seed=6), extent)
    xyz = _cloud(cells, seed=6)
    bad = np.random.default_rng(6).choice(np.arange(1, n), size=TILE + 300, replace=False)   # more than a tile of them: whole tiles without a valid key
    xyz[bad[0::3], 0] = np.nan
    xyz[bad[1::3], 1] = np.inf
    xyz[bad[2::3], 2] = -np.inf
    t, exp = _check(gpu, xyz, layout)
    assert exp["nf"] == n - bad.size and t["start"][-1] == exp["nf"]
