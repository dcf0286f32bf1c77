"""The numpy references of the segment tables (tests/helpers.py: ref_descriptors, ref_features, graph_truth, segment_limits) against slow,
obvious restatements on small random inputs -- labels that occur once, labels that never occur, dropped points, NaN weights, a segment of
one node, zeros of both signs -- so that a bug in a reference cannot hide a bug in a kernel; and the scenes of tests/segment_scenes.py
on the CPU oracle: the merge-rule knobs at a small size, and the NaN weights of the two tilted planes in the reference's arithmetic.
No GPU."""
import numpy as np
import pytest

from helpers import SD_CHUNK, graph_truth, ref_descriptors, ref_features, same_box, segment_limits
from segment_scenes import FAR, GROUP, SPLIT, big_nodes, degenerate_scene, fragmented_plane, thin_segment, two_tilted_planes


# ---------------------------------------------------------------- descriptors
def _cloud(seed, n=400, K=9, shift=0.0):
    """Points with labels -1 .. K-3; label 3 and label K-1 never occur, label K-2 occurs once."""
    rng = np.random.default_rng(seed)
    xyz = (rng.normal(0.0, 1.0, (n, 3)) * rng.uniform(0.01, 3.0, 3) + shift).astype(np.float32)
    labels = rng.integers(-1, K - 2, n).astype(np.int32)
    labels[labels == 3] = 4
    labels[7] = K - 2
    return xyz, labels, K


@pytest.mark.parametrize("seed,shift", [(1, 0.0), (2, 0.0), (3, 1e5)])
def test_ref_descriptors_against_a_loop_per_segment(seed, shift):
    xyz, labels, K = _cloud(seed, shift=shift)
    ref = ref_descriptors(xyz, labels, K)
    seen = set()
    for k in range(K):
        p = xyz[labels == k]
        assert ref["n_points"][k] == p.shape[0]
        seen.add(min(p.shape[0], 2))
        if p.shape[0] == 0:
            assert (ref["bbox6"][k, :3] == np.inf).all() and (ref["bbox6"][k, 3:] == -np.inf).all()
            assert np.isnan(ref["centroid3"][k]).all() and np.isnan(ref["cov6"][k]).all() and np.isnan(ref["evals3"][k]).all()
            continue
        box = np.concatenate([p.min(axis=0), p.max(axis=0)])
        assert np.array_equal(ref["bbox6"][k].view(np.uint32), box.view(np.uint32))
        x = p.astype(np.float64)
        mean = x.mean(axis=0)
        C = np.cov(x, rowvar=False, bias=True) if x.shape[0] > 1 else np.zeros((3, 3))
        assert (np.abs(ref["centroid3"][k] - mean) <= 1e-12 * (1 + np.abs(mean))).all()
        cov6 = C[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
        assert (np.abs(ref["cov6"][k] - cov6) <= 1e-10 * np.trace(C) + 1e-300).all()
        w, v = np.linalg.eigh(C)
        assert (np.abs(ref["evals3"][k] - w) <= 1e-10 * max(w[2], 0.0) + 1e-300).all()
        for j in range(3):
            gap = min(abs(w[j] - w[j - 1]) if j > 0 else np.inf, abs(w[j + 1] - w[j]) if j < 2 else np.inf)
            if gap >= 1e-3 * w[2]:
                assert abs(ref["evecs"][k, :, j] @ v[:, j]) >= 1 - 1e-9
    assert seen == {0, 1, 2}   # labels that never occur, occur once, occur often


def test_ref_features_against_the_oracle(oracle):
    """ref_features against the oracle's vm_eigen_features (DevMath) row by row: random spectra, zeros, ties."""
    rng = np.random.default_rng(4)
    ev = np.sort(rng.uniform(0.0, 2.0, (200, 3)) ** 3, axis=1)
    ev[:20, 0] = 0
    ev[20:40, :2] = 0
    ev[40:45] = 0
    ev[45:60, 1] = ev[45:60, 2]
    ev[60:70, :] = ev[60:70, 2:3]
    ev = ev.astype(np.float32)
    for svgs in (False, True):
        F = ref_features(ev, svgs)
        for i in range(ev.shape[0]):
            np.testing.assert_allclose(F[i], oracle.eigen_features(ev[i], svgs=svgs, math=1), rtol=1e-5, atol=1e-6, err_msg=str((svgs, i)))


def test_zero_signs_of_the_box():
    """A zero bound may carry either sign only in a coordinate where the segment holds both +0.0 and -0.0."""
    xyz = np.array([[0.0, 1.0, -0.0], [-0.0, 2.0, -0.0], [1.0, 0.0, 1.0], [0.0, -1.0, 0.0], [2.0, 0.0, 3.0]], dtype=np.float32)
    labels = np.array([0, 0, 0, 1, 1], dtype=np.int32)
    ref = ref_descriptors(xyz, labels, 2)
    # segment 0: x holds +0 and -0 (min x), z only -0 (min z); segment 1: only +0 (min z, max y irrelevant)
    assert ref["zero_signs"].tolist() == [[True, False, False, True, False, False], [False, False, False, False, False, False]]
    flipped = ref["bbox6"].copy()
    flipped[0, 0] = -flipped[0, 0]
    assert same_box(flipped, ref["bbox6"], ref["zero_signs"])            # min x of segment 0: either sign
    for k, f in ((0, 2), (1, 2)):                                        # min z: one sign only in its segment
        flipped = ref["bbox6"].copy()
        flipped[k, f] = -flipped[k, f]
        assert not same_box(flipped, ref["bbox6"], ref["zero_signs"]), (k, f)


# ---------------------------------------------------------------- graph
def _graph_case(seed, V=70, K=12, big=0):
    """Random symmetric rows (some holding their own node, in any order), labels -1 .. K-3 (label 5 and K-1 never occur, K-2 on one node;
    `big` added to every label and to K, for keys above 2^32), weights with NaN, the pairs between labels 0 and 1 all NaN."""
    rng = np.random.default_rng(seed)
    A = rng.random((V, V)) < 0.2
    A = A | A.T
    np.fill_diagonal(A, rng.random(V) < 0.5)
    rows = [rng.permutation(np.nonzero(A[u])[0]) for u in range(V)]
    off = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    idx = np.concatenate(rows).astype(np.int32)
    lab = rng.integers(-1, K - 2, V)
    lab[lab == 5] = 6
    lab[3] = K - 2
    W = rng.random((V, V)).astype(np.float32)
    W[rng.random((V, V)) < 0.3] = np.nan
    W[np.ix_(lab == 0, lab == 1)] = np.nan
    W[np.ix_(lab == 1, lab == 0)] = np.nan
    lab = np.where(lab >= 0, lab + big, -1)
    return lab, rows, off, idx, K + big, W


def _slow_graph(lab, rows, W):
    """Straight from include/vgs.h: every node pair {u, v} with v in u's row, both labelled, labels a < b."""
    E = {}
    for u, row in enumerate(rows):
        for v in row.tolist():
            if v <= u or lab[u] < 0 or lab[v] < 0 or lab[u] == lab[v]:
                continue
            a, b = sorted((int(lab[u]), int(lab[v])))
            e = E.setdefault((a, b), dict(n=0, f=0, s=0.0, lo=np.inf, hi=-np.inf, A=set(), B=set()))
            e["n"] += 1
            for x in (u, v):
                (e["A"] if lab[x] == a else e["B"]).add(x)
            w = W[u, v]
            if not np.isnan(w):
                e["f"] += 1
                e["s"] += float(w)
                e["lo"], e["hi"] = min(e["lo"], w), max(e["hi"], w)
    return dict(sorted(E.items()))


@pytest.mark.parametrize("seed,big", [(1, 0), (2, 0), (3, 70_000)])
def test_graph_truth_against_a_double_loop(seed, big):
    lab, rows, off, idx, K, W = _graph_case(seed, big=big)
    slow = _slow_graph(lab, rows, W)
    t = graph_truth(lab, off, idx, K, lambda a, b: W[a, b])
    assert [tuple(r) for r in t["seg_ab"].tolist()] == list(slow)
    assert t["n_pairs"].tolist() == [e["n"] for e in slow.values()]
    assert t["n_finite"].tolist() == [e["f"] for e in slow.values()]
    assert t["nodes_ab"].tolist() == [[len(e["A"]), len(e["B"])] for e in slow.values()]
    assert np.allclose(t["w_sum"], [e["s"] for e in slow.values()], rtol=1e-12, atol=0)
    lo = np.array([e["lo"] if e["f"] else np.nan for e in slow.values()], dtype=np.float32)
    hi = np.array([e["hi"] if e["f"] else np.nan for e in slow.values()], dtype=np.float32)
    assert np.array_equal(t["w_min"].view(np.uint32), lo.view(np.uint32)) and np.array_equal(t["w_max"].view(np.uint32), hi.view(np.uint32))
    # the case holds what it is for: NaN weights, an edge without a finite one, a segment of one node, keys above 2^32 when big
    f = t["n_finite"]
    assert ((f > 0) & (f < t["n_pairs"])).any() and (f == 0).any()
    assert (lab == K - 2).sum() == 1 and (t["seg_ab"] == K - 2).any()
    assert t["key"].max() >= 2 ** 32 if big else True
    # the limits it reports
    A = {u: {int(lab[v]) for v in rows[u].tolist() if lab[v] >= 0 and lab[v] != lab[u]} for u in range(len(rows)) if lab[u] >= 0}
    lim = segment_limits(K, np.repeat(lab, 3), truth=t, graph=t)
    assert lim["max_row_labels"] == max(len(s) for s in A.values())
    assert lim["max_edge_records"] == max(len(e["A"]) + len(e["B"]) for e in slow.values())
    assert lim["max_key"] == max(a * K + b for a, b in slow)
    assert lim["nan_edges"] == sum(0 < e["f"] < e["n"] for e in slow.values())
    assert lim["no_finite_edges"] == sum(e["f"] == 0 for e in slow.values())
    # weights of a sample only: the same values on the sampled rows
    for sample in (5, np.array([3, 0, 3])):
        s = graph_truth(lab, off, idx, K, lambda a, b: W[a, b], sample=sample)
        ws = s["wsel"]
        assert ws.size == (5 if np.ndim(sample) == 0 else 2)
        for k in ("n_finite", "w_sum", "w_min", "w_max"):
            assert np.array_equal(s[k][ws].view(np.uint8), t[k][ws].view(np.uint8)), k


def test_graph_truth_without_edges():
    lab = np.array([0, 0, -1, 1])
    off = np.array([0, 2, 4, 5, 6])
    idx = np.array([0, 1, 0, 1, 2, 3])   # node 3 touches only itself, node 2 is unlabelled
    t = graph_truth(lab, off, idx, 2, lambda a, b: np.zeros(a.shape, np.float32))
    assert t["seg_ab"].shape == (0, 2) and t["n_pairs"].shape == (0,) and t["wsel"].shape == (0,)


def test_segment_limits_of_a_hand_made_layout():
    # segment 0: nodes 0 and 2 of 2048 points (node 2 starts chunk 1); segment 1: node 1 of 4097 (three chunks), then node 3 of one point;
    # segment 2: nodes 4 and 6; node 5 dropped
    node_label = np.array([0, 1, 0, 1, 2, -1, 2])
    node_points = np.array([2048, 4097, 2048, 1, 5, 9, 2043])
    pl = np.repeat(node_label, node_points)
    lim = segment_limits(3, pl, node_label, node_points)
    assert lim["seg_points"].tolist() == [4096, 4098, 2048] and lim["seg_mod"].tolist() == [0, 2, 0]
    assert lim["max_node_points"] == 4097 and lim["first_node_chunks"] == 3 and lim["nodes_on_chunk_start"] == 1
    # four nodes of 1024: the third starts chunk 1
    lim = segment_limits(1, np.zeros(4096, np.int32), np.zeros(4, np.int64), np.full(4, 1024))
    assert lim["nodes_on_chunk_start"] == 1 and lim["first_node_chunks"] == 1 and lim["seg_mod"].tolist() == [0]
    assert SD_CHUNK == 2048


# ---------------------------------------------------------------- the knobs of the GPU limit scenes, on the oracle
def test_merge_rule_knobs_on_the_oracle(oracle):
    # cut_thred = 0: every used voxel its own segment, here with rows of about 145 entries
    r = oracle.run_vgs(fragmented_plane(side=24), oracle.vgs_params(graph_size=0.7, **SPLIT))
    assert r.used_nodes == r.kept_clusters == 24 * 24
    # cut_thred = 100: one segment per group, also far from the origin (no NaN weight between voxels of <= 3 points)
    groups = ([2047], [2048, 2048], [1024, 1024, 1024, 1024, 1], [3, 45])
    r = oracle.run_vgs(big_nodes(groups=groups), oracle.vgs_params(**GROUP))
    pl, _ = r.labels()
    assert sorted(np.bincount(pl[pl >= 0]).tolist()) == sorted([1] + [sum(g) for g in groups])
    for shift in (None, FAR):
        xyz, first = degenerate_scene(shift)
        pl, _ = oracle.run_vgs(xyz, oracle.vgs_params(**GROUP)).labels()
        assert (pl >= 0).all() and np.unique(pl).size == len(first)
        assert all(np.unique(pl[a:b]).size == 1 for a, b in zip(first.values(), list(first.values())[1:] + [xyz.shape[0]]))
    pl, _ = oracle.run_vgs(thin_segment(), oracle.vgs_params(**GROUP)).labels()
    assert (pl == 0).all()


def test_nan_scene_on_the_oracle(oracle):
    """two_tilted_planes, the scene of test_gpu_segment_limits.py::test_nan_weights, on the oracle's nodes, rows and labels: edges with some
    NaN pair weights in the reference's own arithmetic (RefMath: libm acos, no clamp) and in the device's (DevMath), and in DevMath also
    edges whose every pair weight is NaN."""
    xyz = two_tilted_planes()
    r = oracle.run_vgs(xyz, oracle.vgs_params(voxel_size=0.1))
    nd = r.nodes()
    off, idx = r.lists("adjacency")
    pl, _ = r.labels()
    pv = r.voxel_table()["point_voxel"]
    lab = np.full(r.V, -1, dtype=np.int64)
    lab[pv[pl >= 0]] = pl[pl >= 0]
    lab[~nd["used"].astype(bool)] = -1
    n16 = [oracle.node16(nd["centroid"][v], nd["normal"][v], nd["eigen"][v]) for v in range(r.V)]
    out = {}
    for math in (0, 1):
        p = oracle.vgs_params(voxel_size=0.1, math=math)
        t = graph_truth(lab, off, idx, int(pl.max()) + 1,
                        lambda a, b: np.array([oracle.pair_weight(n16[x], n16[y], p) for x, y in zip(a.tolist(), b.tolist())], np.float32))
        f, n = t["n_finite"], t["n_pairs"]
        out[math] = (int(((f > 0) & (f < n)).sum()), int((f == 0).sum()))
    assert out[0][0] > 0 and out[1][0] > 0 and out[1][1] > 0, out
