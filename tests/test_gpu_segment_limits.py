"""The segment tables at their structural limits -- the branches of csrc/segdesc.hip and csrc/seggraph.hip that natural scenes do not
reach -- against the numpy references of tests/helpers.py, each case asserting through segment_limits / engine_limits that it reached
the limit it is named for:
  * a fragmented plane: K > 65 536 segments (edge sort keys above 2^32) and rows with more than 128 distinct boundary labels;
  * a 150 m wall on a ground strip: one edge of more than 64 * 256 records, checked over all its pairs;
  * two exact tilted planes, where the unclamped acos makes some pair weights NaN: edges with some and with no finite weight;
  * nodes larger than a descriptor chunk (2 048 points): segments just below, on and above its multiples, a node that starts a chunk,
    a first node over three chunks; the same with stride-16 input and with non-finite points mixed in;
  * degenerate segments (1-3 points, collinear, coplanar, a cube's corners, identical points) near the origin and 3e5 / 5e5 m away;
  * a thin 100 m segment far from the origin, its smallest eigenvalue against its own value;
  * +0.0 and -0.0 at box bounds;
  * determinism at the first two limits.
  * the fragmented plane and the large nodes again across four ranks of the native tiled driver (2 x 2, ranks as threads), against
    numpy over the gathered points, with tens of thousands of moment records per rank in its variable-length all-gather.
The scenes and the parameters that make their segmentation known in advance are in tests/segment_scenes.py."""
import numpy as np
import pytest

from helpers import (SD_CHUNK, check_descriptors, check_graph, engine_limits, graph_inputs, graph_truth, pair_weights, ref_descriptors,
                     ref_graph)
from segment_scenes import (BIG_NODES, DEGENERATE, FAR, GROUP, Q, SIGNED_ZEROS, SPLIT, big_nodes, degenerate_scene, fragmented_plane,
                            thin_segment, two_tilted_planes, wall_on_ground)

pytestmark = pytest.mark.gpu


def _engine(gpu, xyz, **kw):
    eng = gpu.Engine(gpu.default_params(2, **kw))
    eng.set_points(xyz)
    eng.run()
    return eng


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def _report(name, lim):
    print(f"LIMITS {name}: " + ", ".join(f"{k}={v}" for k, v in lim.items() if np.ndim(v) == 0))


# ---------------------------------------------------------------- many segments, many labels per row
@pytest.fixture(scope="module")
def plane(gpu):
    xyz = fragmented_plane()
    return xyz, _engine(gpu, xyz, graph_size=0.7, **SPLIT)


def test_many_segments_and_labels_per_row(gpu, plane):
    """K > 65 536: edge keys min * K + max above 2^32 (the sort's bit count); graph_size = 7 voxels: rows of about 145 entries, every one
    a label of its own (the row walk, once per distinct label, in chunks of 64 entries)."""
    xyz, eng = plane
    c = eng.counts()
    assert c["kept"] == c["used"]   # nothing merged
    truth = ref_graph(eng, sample=300)
    got = check_graph(eng, ref=truth)
    lim = engine_limits(eng, truth=truth)
    _report("many_segments", lim)
    assert lim["K"] > 65_536 and got["seg_ab"].shape[0] > 0
    assert lim["max_key"] >= 2 ** 32
    assert lim["max_row_labels"] > 128
    check_descriptors(eng, xyz, svgs=False)


def test_deterministic_at_many_segments(gpu, plane):
    xyz, eng = plane
    g, d = eng.segment_graph(), eng.segment_descriptors()
    assert _same(g, eng.segment_graph()) and _same(d, eng.segment_descriptors())
    e2 = _engine(gpu, xyz, graph_size=0.7, **SPLIT)
    assert _same(g, e2.segment_graph()) and _same(d, e2.segment_descriptors())


# ---------------------------------------------------------------- one edge of many records
def test_one_edge_of_many_records(gpu):
    """The wall against the ground: more than 64 * 256 records (several chunks of k_sg_chunks, and k_sg_final's lane-stride loop more
    than once); that edge's n_pairs, nodes_ab, w_sum, w_min and w_max over all of its pairs, counts of every edge exact."""
    xyz = wall_on_ground()
    eng = _engine(gpu, xyz, voxel_size=0.1, graph_size=0.5, points_min=3)
    lab, off, idx, K = graph_inputs(eng)
    counts = graph_truth(lab, off, idx, K)
    E = counts["seg_ab"].shape[0]
    big = int(np.argmax(counts["nodes_ab"].astype(np.int64).sum(axis=1)))
    sample = np.append(np.random.default_rng(0).choice(E, size=min(100, E), replace=False), big)
    truth = graph_truth(lab, off, idx, K, lambda a, b: pair_weights(eng, a, b), sample=sample)
    assert big in truth["wsel"]
    got = check_graph(eng, ref=truth)
    lim = engine_limits(eng, truth=truth)
    _report("one_edge_of_many_records", lim)
    assert lim["max_edge_records"] > 64 * 256
    assert truth["n_finite"][big] > 0


# ---------------------------------------------------------------- NaN weights
def test_nan_weights(gpu):
    """Two exact tilted planes 0.45 m apart: the voxels of a plane hold the same lattice, so their float normals agree to the last bits
    and the dot product of two of them lands on either side of 1 -- the unclamped acos gives NaN for some pairs and not for others (the
    oracle on the same scene, tests/test_segment_refs_cpu.py::test_nan_scene_on_the_oracle: partly-NaN edges with its RefMath weight, and
    with DevMath partly-NaN edges and all-NaN edges).  Edges with some
    finite weights and edges with none (w_min = w_max = NaN, w_sum = 0); every edge's weights are checked."""
    xyz = two_tilted_planes()
    eng = _engine(gpu, xyz, voxel_size=0.1)
    truth = ref_graph(eng)
    got = check_graph(eng, ref=truth)
    lim = engine_limits(eng, truth=truth, graph=got)
    _report("nan_weights", lim)
    assert lim["nan_edges"] > 0 and lim["no_finite_edges"] > 0
    none = got["n_finite"] == 0
    assert np.isnan(got["w_min"][none]).all() and np.isnan(got["w_max"][none]).all() and (got["w_sum"][none] == 0).all()
    some = ~none
    assert not np.isnan(got["w_min"][some]).any() and not np.isnan(got["w_max"][some]).any()


# ---------------------------------------------------------------- nodes larger than a descriptor chunk
@pytest.fixture(scope="module")
def nodes_scene(gpu):
    xyz = big_nodes()
    return xyz, _engine(gpu, xyz, **GROUP)


def test_nodes_larger_than_a_chunk(gpu, nodes_scene):
    xyz, eng = nodes_scene
    got = check_descriptors(eng, xyz, svgs=False)
    lim = engine_limits(eng)
    _report("nodes_larger_than_a_chunk", lim)
    assert sorted(lim["seg_points"].tolist()) == sorted([1] + [sum(g) for g in BIG_NODES])   # one segment per group
    assert sorted(got["n_nodes"].tolist()) == sorted([1] + [len(g) for g in BIG_NODES])
    assert lim["max_node_points"] >= 10_000
    assert lim["first_node_chunks"] >= 3          # a first node over three chunks; [10000]: a segment of one node in five chunks
    assert lim["nodes_on_chunk_start"] >= 1       # a node boundary on a chunk boundary
    assert {0, 1, SD_CHUNK - 1} <= set(lim["seg_mod"].tolist())


def test_input_forms_at_the_node_limits(gpu, nodes_scene):
    """Stride-16 input, and non-finite points mixed in: up to renaming, the same table as the stride-12 finite run, byte for byte."""
    xyz, eng = nodes_scene
    base, la = eng.segment_descriptors(), eng.point_labels()
    K = base["n_points"].shape[0]
    rng = np.random.default_rng(5)
    xyz4 = np.concatenate([xyz, rng.uniform(0.0, 1.0, (xyz.shape[0], 1)).astype(np.float32)], axis=1)
    bad = np.array([[np.nan, 0, 0], [np.inf, 1, 1], [0, -np.inf, 0], [1, 1, np.nan]], dtype=np.float32)
    at = np.sort(rng.choice(np.arange(1, xyz.shape[0]), size=64, replace=False))   # never first: the first point pins the grid
    xyzn = np.insert(xyz, at, bad[np.arange(64) % 4], axis=0)
    finite = np.isfinite(xyzn).all(axis=1)
    for cloud, keep in ((xyz4, slice(None)), (xyzn, finite)):
        e = _engine(gpu, cloud, **GROUP)
        lab = e.point_labels()
        if keep is finite:
            assert (lab[~finite] < 0).all()
        lab = lab[keep]
        m = la >= 0
        assert np.array_equal(m, lab >= 0)
        p = np.full(K, -1, dtype=np.int64)
        p[la[m]] = lab[m]
        assert np.array_equal(p[la[m]], lab[m]) and np.array_equal(np.sort(p), np.arange(K))   # a renaming
        d = e.segment_descriptors()
        for k in base:
            assert np.array_equal(d[k][p].view(np.uint8), base[k].view(np.uint8)), k
        check_descriptors(e, cloud, svgs=False)


def test_deterministic_at_the_node_limits(gpu, nodes_scene):
    xyz, eng = nodes_scene
    d, g = eng.segment_descriptors(), eng.segment_graph()
    assert _same(d, eng.segment_descriptors()) and _same(g, eng.segment_graph())
    e2 = _engine(gpu, xyz, **GROUP)
    assert _same(d, e2.segment_descriptors()) and _same(g, e2.segment_graph())


# ---------------------------------------------------------------- degenerate geometry, thin segments, signed zeros
@pytest.mark.parametrize("far", [False, True], ids=["origin", "far"])
def test_degenerate_segments(gpu, far):
    xyz, first = degenerate_scene(FAR if far else None)
    eng = _engine(gpu, xyz, **GROUP)
    got = check_descriptors(eng, xyz, svgs=False)
    labels = eng.point_labels()
    k = {name: int(labels[i]) for name, i in first.items()}
    assert eng.counts()["kept"] == len(first) and len(set(k.values())) == len(first)   # one segment per group
    for name, g in DEGENERATE.items():
        assert got["n_points"][k[name]] == len(g), name
    V = got["evecs9"].reshape(-1, 3, 3)
    ev = got["evals3"]
    # n identical points: zero covariance, eigenvalues and features, identity eigenvectors
    s = k["same"]
    assert (got["cov6"][s] == 0).all() and (ev[s] == 0).all() and (got["eigen8"][s] == 0).all() and (V[s] == np.eye(3)).all()
    # along (1, 1, 0) / sqrt 2: an eigenvector whose two largest components tie exactly; the sign rule makes the lower index positive
    s = k["line_xy"]
    tie = [j for j in range(3) if abs(V[s, 0, j]) == abs(V[s, 1, j]) and abs(V[s, 0, j]) > abs(V[s, 2, j])]
    assert tie and all(V[s, 0, j] > 0 for j in tie)
    assert any(V[s, 0, j] * V[s, 1, j] < 0 for j in tie)   # the tie of opposite signs, where "lowest index" decides
    # a cube's corners: a triple eigenvalue
    s = k["cube"]
    assert ev[s, 0] > 0 and ev[s, 2] - ev[s, 0] <= 1e-12 * ev[s, 2]
    # collinear: two zero eigenvalues; coplanar (and three points): one
    for name, zeros in (("two", 2), ("line_x", 2), ("line_xy", 2), ("plane", 1), ("three", 1)):
        s = k[name]
        assert (ev[s, :zeros] <= 1e-12 * ev[s, 2]).all() and ev[s, zeros] > 0, name


def test_thin_long_segment_far_from_the_origin(gpu):
    """100 m long, 5 cm radius, tilted, at (3e5, 5e5, 50) m, the anchor (the segment's first point) at one end: lambda_0 is about 1.5e-6 of
    lambda_max, so check_descriptors' bar of 1e-8 lambda_max allows an error of about 1 % of it.  Here lambda_0 and lambda_1 within 1e-6
    of their own two-pass numpy values.  The radius is 5 cm, not 1 mm: at 5e5 m float32 points lie 6.25 cm apart, so a 1 mm radius would
    be rounded away and lambda_0 would measure the rounding, not the cylinder."""
    xyz = thin_segment()
    eng = _engine(gpu, xyz, **GROUP)
    labels = eng.point_labels()
    assert eng.counts()["kept"] == 1 and (labels == 0).all()
    got = check_descriptors(eng, xyz, svgs=False)
    lam = ref_descriptors(xyz, labels, 1)["evals3"][0]
    assert 0 < lam[0] < 1e-5 * lam[2]
    assert abs(got["evals3"][0, 0] - lam[0]) <= 1e-6 * lam[0], (got["evals3"][0], lam)
    assert abs(got["evals3"][0, 1] - lam[1]) <= 1e-6 * lam[1], (got["evals3"][0], lam)


def test_signed_zeros_at_box_bounds(gpu):
    """A segment whose min x, max y and min z are zeros of both signs: include/vgs.h lets such a bound carry either sign, so those entries
    compare by value (helpers.same_box) and every other entry stays bit-exact."""
    xyz, first = degenerate_scene()
    eng = _engine(gpu, xyz, **GROUP)
    got = check_descriptors(eng, xyz, svgs=False)
    k = int(eng.point_labels()[first["signed_zeros"]])
    z = np.array(SIGNED_ZEROS, dtype=np.float32)
    for axis in (0, 1, 2):   # the input holds both signs of zero in every coordinate
        assert np.signbit(z[z[:, axis] == 0, axis]).any() and (~np.signbit(z[z[:, axis] == 0, axis])).any()
    assert ref_descriptors(xyz, eng.point_labels(), eng.counts()["kept"])["zero_signs"][k].all()   # both signs in x, y and z
    box = got["bbox6"][k]
    assert box[0] == 0 and box[4] == 0 and box[2] == 0
    assert box[3] == Q and box[1] == -Q and box[5] == Q


# ---------------------------------------------------------------- across the ranks of the tiled driver
def _split(xyz, center):
    """2 x 2 tiles around `center`: rank i + 2 j holds the points with x on side i and y on side j, in input order (the first point stays
    the first of rank 0)."""
    sx, sy = xyz[:, 0] >= center[0], xyz[:, 1] >= center[1]
    return [xyz[(sx == bool(i)) & (sy == bool(j))] for j in (0, 1) for i in (0, 1)]


def _tiled(gpu, xyz, center, pitch, params):
    """The scene through the native driver, 2 x 2 ranks as threads: every rank's table the same bytes, call after call and run after run,
    and equal to numpy over the gathered points (test_gpu_tiles_segdesc.py's checks); per rank the number of moment records it puts into
    the descriptor all-gather (128 bytes each)."""
    from test_gpu_tiles_segdesc import _check_against_points, _collect, _ranks
    parts = _split(xyz, center)
    assert np.array_equal(parts[0][0], xyz[0])

    def body(r, t, p):
        o = _collect(r, t, p)
        o["records"] = t.own_segment_moments(o["kept"])["label"].shape[0]
        return o
    out = _ranks(gpu, (2, 2), pitch, parts, body, center=center, params=params)
    d = _check_against_points(gpu, parts, out, params=params)
    return parts, out, d


def test_tiled_many_segments(gpu):
    """The fragmented plane over four ranks (the tile borders cut through voxels): K > 65 536 global segments, and every rank sends a
    moment record for each label it holds -- more than 10 000 records (1.28 MB) per rank in the variable-length all-gather."""
    xyz = fragmented_plane()
    parts, out, d = _tiled(gpu, xyz, (13.65, 13.65), 30.0, gpu.default_params(2, graph_size=0.7, **SPLIT))
    K = out[0]["kept"]
    print(f"LIMITS tiled_many_segments: K={K}, records per rank={[o['records'] for o in out]}")
    assert K > 65_536
    for r, o in enumerate(out):
        own = np.unique(o["labels"][o["labels"] >= 0]).size
        assert o["records"] >= own >= 10_000, (r, o["records"], own)


def test_tiled_nodes_larger_than_a_chunk(gpu):
    """The large nodes over four ranks, the border x = 0.05 m through the middle of every group's first voxel: nodes of up to 10 000 points
    whose points two ranks share, so the own-point chunks (k_sd_chunks_own) filter inside chunks that split such a node."""
    xyz = big_nodes()
    parts, out, d = _tiled(gpu, xyz, (0.05, 22.5), 50.0, gpu.default_params(2, **GROUP))
    assert sorted(d["n_points"].tolist()) == sorted([1] + [sum(g) for g in BIG_NODES])   # one segment per group
    labels = np.concatenate([o["labels"] for o in out])
    rank_of = np.repeat(np.arange(4), [p.shape[0] for p in parts])
    big = np.nonzero((d["n_points"] == 10_000) & (d["n_nodes"] == 1))[0]
    assert big.size == 1
    assert np.unique(rank_of[labels == big[0]]).size == 2   # the 10 000-point node lies on two ranks
    split = [k for k in range(d["n_points"].size) if np.unique(rank_of[labels == k]).size > 1]
    assert len(split) == len(BIG_NODES)
