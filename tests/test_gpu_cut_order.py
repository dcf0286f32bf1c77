"""The reference-order connect lists (csrc/cutorder.hip: k_co_count, k_co_eval, the segmented sort, k_co_merge; k_co_list_count / _fill;
the host's closestCheck appends; the host walk of vgs_get_clusters_ordered) at the limits of the replay kernels, on scenes built for them
(tests/cut_order_scenes.py; VGS, voxel_size 0.0625, graph_size 0.51, everything else default).  Every list is compared element for
element with the CPU oracle or with tests/cut_order_ref.py, which tests/test_cut_order_ref_cpu.py pins to the oracle.

What the scenes hold, checked on the CPU with the oracle (lean flavour) or the restatement; every test asserts its own claim again:
  wide        17 x 17 x 17 parallel sheet voxels: rows of up to 2301 stored entries, 251 above 2048, and for 134 voxels the connect list
              holds a member at row position 2048 or above (up to 2202) -- positions the replay kernels could not index before their LDS
              arrays went from row positions to positions inside the connect set.  The whole oracle takes minutes here, so the C oracle's
              cut runs on the engine's own matrix (Engine.local_weights) of 16 such voxels and 8 with short rows.
  steps       9 x 9 x 9 of the same: connect lists of 1 .. 148 voxels, median 75 (48 below 64, 679 in 64 .. 127, 2 from 128), 135 lists
              shortened by crossValidation, 30 of them losing an entry at list position 64 or above that a kept entry follows (the
              ballot compaction of k_co_list_fill across a 64-entry step), 728 lists whose k (k - 1) / 2 is no multiple of 64 (the last
              partial fetch of k_co_merge), 2 voxels re-attached.  Whole oracle: 6 s on 8 cores.
  singletons  216 sheet voxels six cells apart with turned normals: no pair above 0.641 (1 - cut_thred = 0.7), every list is the voxel
              alone, the chunk's pair total is 0 and the sort is skipped.  closestCheck attaches a lone voxel only to a voxel whose list
              holds more than one entry, so this scene re-attaches none; "singletons+group" adds a 4 x 4 patch of connected sheets:
              70 voxels re-attached, connect_final gets its appended entries.  Both hold one voxel per 4 x 4 x 4 brick of the
              adjacency stage's table: as many bricks as voxels, the most a cloud can have.
  ties        a strip of 48 sheet voxels and its mirror image in x = 0: a pair and its mirror image weigh the same to the bit; lists of
              up to 48, and 93 of 96 voxels hold tied pairs inside their list (about 450 tied weight values each), so the order rests
              on the tie rule -- pair id ascending, i.e. row positions.
  nan         6 x 5 x 2 sheet voxels of which two hold the same points moved by whole voxels: bit-identical normals, acos of a dot
              product above 1, a NaN weight; both lie in the connect list of 30 voxels (the zero key and the early stop of k_co_merge).
The chunk border of the segmented sort (more than 2^29 pairs in one call) is not reached by any of them: tests/test_cutorder_arith.py
covers the partition on the host."""
import os

import numpy as np
import pytest

import cut_order_scenes as S
from cut_order_ref import cross_order, cut_order
from helpers import oracle_params, ragged_lists

pytestmark = pytest.mark.gpu

CONNECT = ("connect_cut", "connect_cross", "connect_final")


def _engine(gpu, xyz):
    p = gpu.default_params(2, **S.PARAMS)
    eng = gpu.Engine(p)
    eng.set_points(xyz)
    eng.run()
    assert eng.schedule_counters()["outside_limits"] == 0
    return eng, p


def _oracle(oracle, p, xyz):
    return oracle.run_vgs(xyz, oracle_params(oracle, p, threads=min(os.cpu_count() or 1, 16)))


def _assert_equals_oracle(eng, ref):
    for which in CONNECT:
        off, idx = eng.lists(which, "reference")
        roff, ridx = ref.lists(which)
        np.testing.assert_array_equal(off, roff, err_msg=which)
        np.testing.assert_array_equal(idx, ridx, err_msg=which)
    off, idx = eng.clusters("reference")
    roff, ridx = ref.lists("clusters_points")
    np.testing.assert_array_equal(off, roff)
    np.testing.assert_array_equal(idx, ridx)


def _assert_equals_restatement(eng, p, probes):
    """connect_cut and connect_cross in reference order of every probe against cut_order over Engine.local_weights and cross_order over the
    engine's own voxel-id-order sets."""
    cut_ref = ragged_lists(*eng.lists("connect_cut", "reference"))
    cross_ref = ragged_lists(*eng.lists("connect_cross", "reference"))
    cut_sets = [frozenset(l) for l in ragged_lists(*eng.lists("connect_cut"))]
    for u in probes:
        ids, W = eng.local_weights(u)
        assert ids[0] == u
        want = ids[cut_order(W, p.cut_thred)].tolist()
        assert cut_ref[u] == want, u
        assert frozenset(want) == cut_sets[u], u
        assert cross_ref[u] == cross_order(want, u, cut_sets), u


# ---------------------------------------------------------------- wide
def test_wide_rows_members_beyond_row_position_2048(gpu, oracle):
    eng, p = _engine(gpu, S.block(17))
    n = eng.adjacency_counts()
    assert n.max() > 2048
    cut_sets = [frozenset(l) for l in ragged_lists(*eng.lists("connect_cut"))]
    cut_ref = ragged_lists(*eng.lists("connect_cut", "reference"))
    cross_ref = ragged_lists(*eng.lists("connect_cross", "reference"))

    def check(u, ids, W):
        want = ids[oracle.cut_graph_order(W, p.cut_thred)].tolist()    # the C oracle's scan over the whole row: 2.6 million edges
        assert cut_ref[u] == want, u
        assert frozenset(want) == cut_sets[u], u
        assert cross_ref[u] == cross_order(want, u, cut_sets), u

    far = 0
    highest = 0
    for u in np.argsort(-n, kind="stable")[:120].tolist():      # the longest rows first
        if n[u] <= 2048 or far == 16:
            break
        ids, W = eng.local_weights(u)
        assert ids[0] == u and ids.shape[0] > 2048
        pos = np.flatnonzero(np.isin(ids, np.fromiter(cut_sets[u], dtype=np.int64)))
        assert pos.shape[0] == len(cut_sets[u])
        if pos.max() < 2048:
            continue
        far += 1
        highest = max(highest, int(pos.max()))
        check(u, ids, W)
    assert far == 16, (far, highest)       # voxels whose connect list reaches row position 2048 or beyond
    short = np.flatnonzero((n > 0) & (n < 2048))
    for u in short[np.linspace(0, short.shape[0] - 1, 8).astype(np.int64)].tolist():
        check(u, *eng.local_weights(u))
    # the clusters in reference order: the default order's clusters, each permuted
    off, idx = eng.clusters()
    roff, ridx = eng.clusters("reference")
    np.testing.assert_array_equal(off, roff)
    assert off.shape[0] > 1 and idx.shape[0] > 0
    cl = np.repeat(np.arange(off.shape[0] - 1), np.diff(off))
    np.testing.assert_array_equal(idx[np.lexsort((idx, cl))], ridx[np.lexsort((ridx, cl))])


# ---------------------------------------------------------------- steps of 64
@pytest.fixture(scope="module")
def steps(gpu, oracle):
    xyz = S.block(9)
    eng, p = _engine(gpu, xyz)
    return dict(xyz=xyz, eng=eng, p=p, ref=_oracle(oracle, p, xyz))


def test_steps_of_64_scene_is_what_it_claims(steps):
    ref = steps["ref"]
    cut = ragged_lists(*ref.lists("connect_cut"))
    cross = ragged_lists(*ref.lists("connect_cross"))
    k = np.array([len(l) for l in cut])
    assert (k < 64).any() and ((k > 64) & (k < 128)).any() and (k > 128).any(), np.bincount(k // 64)
    assert ((k * (k - 1) // 2) % 64 != 0).any()
    across = 0
    for c, x in zip(cut, cross):
        kept = np.isin(c, x)
        assert kept.sum() == len(x)
        late = np.flatnonzero(~kept)
        late = late[late >= 64]
        across += bool(late.size and kept[late[0]:].any())
    assert across > 0       # an entry at list position >= 64 dropped by crossValidation, a kept one behind it
    assert sum(len(x) < len(c) for c, x in zip(cut, cross)) > 0


def test_steps_of_64_lists_and_clusters_equal_the_oracles(steps):
    _assert_equals_oracle(steps["eng"], steps["ref"])


def test_repeat_same_bytes(gpu, steps):
    eng = steps["eng"]

    def grab(e):
        out = [a for which in CONNECT for a in e.lists(which, "reference")]
        return out + list(e.clusters("reference"))

    first = grab(eng)
    for a, b in zip(first, grab(eng)):                 # a second call of each getter
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    eng2, _ = _engine(gpu, steps["xyz"])               # a second fresh Engine
    for a, b in zip(first, grab(eng2)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- singletons
@pytest.mark.parametrize("group", [False, True], ids=["singletons", "singletons+group"])
def test_singletons(gpu, oracle, group):
    """(Every voxel of the lattice is also the only one of its 4 x 4 x 4 brick: as many bricks as voxels.  The adjacency stage's brick table,
    sized by half the voxels until this scene was run, filled up on it and k_brick_insert never found a free slot.)"""
    xyz = S.singletons(group=group)
    eng, p = _engine(gpu, xyz)
    c = eng.counts()
    assert c["used"] == c["voxels"] == (232 if group else 216)
    lists = ragged_lists(*eng.lists("connect_cut", "reference"))
    alone = [u for u, l in enumerate(lists) if l == [u]]
    n = eng.adjacency_counts()
    assert n.min() >= 4                                 # every voxel has neighbours: the lists are short because no pair weighs enough
    if group:
        assert len(alone) == 216 and c["reattached"] > 0, (len(alone), c)
    else:
        assert len(alone) == 216 and c["reattached"] == 0, (len(alone), c)    # every k is 1: no pair, no key, the sort is skipped
    _assert_equals_oracle(eng, _oracle(oracle, p, xyz))
    if group:
        cross = ragged_lists(*eng.lists("connect_cross", "reference"))
        final = ragged_lists(*eng.lists("connect_final", "reference"))
        grown = [u for u in range(len(final)) if len(final[u]) > len(cross[u])]
        assert grown and all(final[u][:len(cross[u])] == cross[u] for u in grown)     # closestCheck appends behind


# ---------------------------------------------------------------- ties
def test_ties_between_mirror_images_follow_the_pair_id(gpu, oracle):
    xyz = S.mirrored()
    eng, p = _engine(gpu, xyz)
    assert eng.counts()["used"] == 96
    cen = eng.attributes()["centroid"]
    cut_sets = [frozenset(l) for l in ragged_lists(*eng.lists("connect_cut"))]
    tied = 0
    for u in np.flatnonzero(np.abs(cen[:, 0]) < S.RES).tolist():       # the voxels on the mirror plane
        ids, W = eng.local_weights(u)
        s0 = np.flatnonzero(np.isin(ids, list(cut_sets[u])))
        a, b = np.triu_indices(s0.shape[0], 1)
        w = W[s0[a], s0[b]]
        bits = w[~np.isnan(w)].view(np.uint32)
        tied += np.unique(bits).shape[0] < bits.shape[0]               # two distinct pairs inside S0 of bit-equal weight
    assert tied > 0
    _assert_equals_restatement(eng, p, range(96))
    _assert_equals_oracle(eng, _oracle(oracle, p, xyz))


# ---------------------------------------------------------------- NaN inside S0
def test_nan_weight_inside_a_connect_set(gpu, oracle):
    xyz, copies = S.translates()
    eng, p = _engine(gpu, xyz)
    V = eng.counts()["voxels"]
    assert eng.counts()["used"] == V == 60
    pv = eng.point_voxel()
    va, vb = (int(pv[1 + i * S.PTS]) for i in copies)
    assert va != vb
    cut_sets = [frozenset(l) for l in ragged_lists(*eng.lists("connect_cut"))]
    both = [u for u in range(V) if va in cut_sets[u] and vb in cut_sets[u]]
    assert both
    ids, W = eng.local_weights(both[0])
    pa, pb = int(np.flatnonzero(ids == va)[0]), int(np.flatnonzero(ids == vb)[0])
    assert np.isnan(W[pa, pb]) and np.isnan(W[pb, pa])                 # a NaN pair inside S0 of every voxel in `both`
    _assert_equals_restatement(eng, p, range(V))
    _assert_equals_oracle(eng, _oracle(oracle, p, xyz))
