"""tests/cut_order_ref.py pinned to the CPU oracle (no GPU): cut_order against the oracle's lean cut with its list left in merge-history
order (refcpu_py.cut_graph_order), over random matrices built for exact ties and NaN entries, and cut_order + cross_order against the
lists of a whole oracle run.  This is what licenses tests/test_gpu_cut_order.py to compare the kernels of csrc/cutorder.hip with either.

The restatement tells these faults apart (each was put into a copy of cut_order and made test_restatement_equals_the_oracles_cut
fail): the tie order reversed (b, a descending), >= for > in the merge test, the survivor chosen by size, the threshold in float64."""
import numpy as np

from cut_order_ref import cross_order, cut_order
from helpers import ragged_lists

CUTS = (0.1, 0.3, 0.9)


def _matrix(rng, n, levels, nan_share, cut=None):
    """A symmetric n x n float32 matrix whose entries come from `levels` distinct values (exact ties abound), some of them NaN.  With
    `cut`, the values also hold 1 and, for every value v, the float32 thresholds v - cut / s of a segment of s = 1 .. 4 vertices whose last
    merge weighed v: weights that EQUAL a threshold the scan will meet (they must not merge), exact only in float32 arithmetic."""
    vals = rng.uniform(0.05, 1.0, levels).astype(np.float32)
    if cut is not None:
        vals = np.concatenate([vals, [np.float32(1)]]).astype(np.float32)
        vals = np.concatenate([vals] + [vals - np.float32(cut) / np.float32(s) for s in (1, 2, 3, 4)]).astype(np.float32)
        levels = vals.shape[0]
    W = vals[rng.integers(0, levels, (n, n))]
    W[rng.random((n, n)) < nan_share] = np.nan
    W = np.triu(W, 1)
    W = W + W.T
    np.fill_diagonal(W, 1.0)
    return W.astype(np.float32)


def test_restatement_equals_the_oracles_cut(oracle):
    rng = np.random.default_rng(5)
    cases = 0
    merged = []
    # most matrices small (the Python scan is a loop over n (n - 1) / 2 edges), every n of 1 .. 300 possible, 150 of them from the upper end
    sizes = np.concatenate([np.arange(1, 61), rng.integers(1, 61, 1900), rng.integers(61, 301, 150), [300, 299, 257, 256, 255]])
    for n in sizes.tolist():
        cut = float(CUTS[cases % 3])
        W = _matrix(rng, n, levels=int(rng.integers(2, 9)), nan_share=float(rng.choice([0.0, 0.05, 0.3, 0.7])),
                    cut=cut if cases % 2 else None)
        got = cut_order(W, cut)
        want = oracle.cut_graph_order(W, cut)
        assert got == want, (n, cut)
        assert 0 in got
        merged.append(len(got))
        cases += 1
    assert cases >= 2000
    merged = np.array(merged)
    assert (merged == 1).sum() > 20 and (merged > 100).sum() > 20, np.bincount(np.minimum(merged, 101))   # both ends occur


def test_the_two_asymmetric_cases(oracle):
    for cut in CUTS:
        assert cut_order(np.ones((1, 1), np.float32), cut) == [0] == oracle.cut_graph_order(np.ones((1, 1), np.float32), cut)
        # nothing merges: every weight at or below the first threshold 1 - cut (equality does not merge), or NaN
        thr0 = np.float32(1) - np.float32(cut) / np.float32(1)
        for n in (2, 3, 17, 64):
            W = np.full((n, n), thr0, dtype=np.float32)
            W[0, 1] = W[1, 0] = np.nan
            W[n - 1, 0] = W[0, n - 1] = np.nextafter(thr0, np.float32(0))
            assert cut_order(W, cut) == [0] == oracle.cut_graph_order(W, cut), (n, cut)
            W[0, n - 1] = np.nextafter(thr0, np.float32(2))   # one edge just above: exactly that pair
            assert cut_order(W, cut) == [0, n - 1] == oracle.cut_graph_order(W, cut), (n, cut)


def test_a_tie_is_scanned_in_pair_order_and_the_absorbed_list_goes_behind(oracle):
    """Hand-made: equal weights merge in (a, b) order, and a later merge appends the absorbed segment's list whole."""
    W = np.full((5, 5), np.nan, dtype=np.float32)
    for a, b, w in ((3, 4, 0.97), (0, 2, 0.96), (0, 1, 0.96), (1, 3, 0.95)):
        W[a, b] = W[b, a] = w
    # (3,4) first: threshold 0.97 - 0.1 / 2 = 0.92; then the tie, (0,1) before (0,2): [0, 1], [0, 1, 2], threshold 0.96 - 0.1 / 3 = 0.9267;
    # then (1,3): 0.95 is above both, the segment of 1 has the higher threshold and survives
    assert cut_order(W, 0.1) == [0, 1, 2, 3, 4] == oracle.cut_graph_order(W, 0.1)
    W[0, 2] = W[2, 0] = 0.965   # no tie any more: (0,2) before (0,1)
    assert cut_order(W, 0.1) == [0, 2, 1, 3, 4] == oracle.cut_graph_order(W, 0.1)
    W[3, 4] = W[4, 3] = 0.99    # threshold of {3, 4} now 0.94 > 0.9267: the segment of 3 survives, the centre's list goes behind it
    assert cut_order(W, 0.1) == [3, 4, 0, 2, 1] == oracle.cut_graph_order(W, 0.1)


def test_whole_scene_lists_from_node_records(oracle, vgs):
    """town_scene(20000), default parameters: W of a used voxel from the oracle's node records and pair_weight; cut_order and cross_order
    over them must give the oracle's connect_cut and connect_cross lists element for element."""
    xyz = vgs.scenes.town_scene(20000)
    rp = oracle.vgs_params(math=1, flavour=1)
    ref = oracle.run_vgs(xyz, rp)
    nd = ref.nodes()
    used = nd["used"].astype(bool)
    n16 = [oracle.node16(nd["centroid"][v], nd["normal"][v], nd["eigen"][v], used=bool(used[v])) for v in range(ref.V)]
    adj = ragged_lists(*ref.lists("adjacency"))
    cut = ragged_lists(*ref.lists("connect_cut"))
    cross = ragged_lists(*ref.lists("connect_cross"))
    cut_sets = [frozenset(l) for l in cut]       # voxel-id order or any other: membership is all crossValidation asks of the other list
    ids_used = np.flatnonzero(used)
    # the voxels with the longest lists and a seeded sample of the rest, small rows only to keep the pair weights few
    by_len = sorted(ids_used.tolist(), key=lambda v: -len(cut[v]))
    rng = np.random.default_rng(3)
    probes = [v for v in by_len if len(adj[v]) <= 80][:60] + rng.choice(ids_used, 400, replace=False).tolist()
    done = shortened = longest = 0
    for u in dict.fromkeys(probes):
        row = adj[u]
        if row[0] != u or len(row) > 80:
            continue
        n = len(row)
        W = np.full((n, n), np.nan, dtype=np.float32)    # an unused neighbour takes no part in the lean cut: as if its weights were NaN
        for a in range(n):
            if not used[row[a]]:
                continue
            for b in range(a + 1, n):
                if used[row[b]]:
                    W[a, b] = oracle.pair_weight(n16[row[a]], n16[row[b]], rp)
        got = [row[r] for r in cut_order(W, rp.cut_thred)]
        assert got == cut[u], u
        gx = cross_order(got, u, cut_sets)
        assert gx == cross[u], u
        done += 1
        shortened += len(gx) < len(got)
        longest = max(longest, len(got))
    assert done >= 200 and shortened > 0 and longest >= 8, (done, shortened, longest)
