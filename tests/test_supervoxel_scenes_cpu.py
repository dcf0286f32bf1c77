"""The scenes of tests/supervoxel_scenes.py on the CPU oracle alone: every scene reaches the path of csrc/vccs.hip or csrc/svgs.hip it was
built for, asserted through the predicates of that module from the oracle's labels and voxel table (the oracle restates the sequential /
per-voxel algorithm without tiles or LDS tables, so what it says about a scene does not depend on the paths under test); the predicates
themselves against brute-force restatements on a small random table; and the contract for non-finite points under a caller's labelling.
No GPU."""
import numpy as np
import pytest

import supervoxel_scenes as S

VT_SLOTS, VX_SLOTS, VTN_CAP = 32, 128, 448   # csrc/vccs.hip


def _rounds(kw):
    """(int)(1.8f * seed / res) in float, as the driver computes it."""
    return int(np.float32(1.8) * np.float32(kw["seed_size"]) / np.float32(kw["voxel_size"]))


_CACHE = {}


def _scene(oracle, name, mode):
    """xyz, parameters, the oracle's labels / max_label / seeds, its voxel table and the voxels' labels -- computed once per scene and mode."""
    if (name, mode) not in _CACHE:
        xyz, kw = S.SUPERVOXEL_SCENES[name]()
        p = oracle.svgs_params(**kw)
        if mode == 0:
            lab, mx = oracle.vccs(xyz, p)
            seeds = mx
        else:
            lab, mx, seeds = oracle.vccs_pcl_seeds(xyz, p)
            lab2, mx2 = oracle.vccs_pcl(xyz, p)
            assert mx2 == mx and np.array_equal(lab, lab2)
        T = oracle.voxelize(xyz, kw["voxel_size"], bbox_first=bool(mode)).voxel_table()
        _CACHE[(name, mode)] = dict(xyz=xyz, kw=kw, lab=lab, mx=mx, seeds=seeds, T=T, vl=S.voxel_labels(T, lab))
    return _CACHE[(name, mode)]


def _report(name, mode, **kw):
    print(f"PATH {name} m{mode}: " + ", ".join(f"{k}={v}" for k, v in kw.items()))


# ---------------------------------------------------------------- the predicates against brute force
def test_predicates_against_brute_force():
    rng = np.random.default_rng(7)
    key = np.unique(rng.integers(5, 23, (4000, 3)), axis=0)
    key = key[np.argsort(S.morton(key))[::-1]].astype(np.uint32)
    V = key.shape[0]
    vlab = rng.integers(0, 40, V)
    xyz = (key.astype(np.float64) + rng.uniform(0.1, 0.9, (V, 3))).astype(np.float32)
    table = dict(key=key, point_voxel=np.arange(V))
    at = {tuple(k): i for i, k in enumerate(key.tolist())}
    tiles = {}
    for i, k in enumerate(key.tolist()):
        tiles.setdefault((k[0] >> 3, k[1] >> 3, k[2] >> 3), []).append(i)
    order = sorted(tiles, key=lambda t: min(tiles[t]))   # tiles in table order
    assert S.labels_per_tile(table, vlab).tolist() == [len({int(vlab[i]) for i in tiles[t]} - {0}) for t in order]
    assert S.labels_per_256(vlab).tolist() == [len(set(vlab[s:s + 256].tolist()) - {0}) for s in range(0, V, 256)]
    per27, own, shell = [], [], []
    for k in key.tolist():
        seen = set()
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    j = at.get((k[0] + dx, k[1] + dy, k[2] + dz))
                    if j is not None:
                        seen.add(int(vlab[j]))
        per27.append(len(seen - {0}))
    assert S.labels_per_27(table, vlab).tolist() == per27
    for t in order:
        own.append(len(tiles[t]))
        n = 0
        for x in range(8 * t[0] - 1, 8 * t[0] + 9):
            for y in range(8 * t[1] - 1, 8 * t[1] + 9):
                for z in range(8 * t[2] - 1, 8 * t[2] + 9):
                    if (x >> 3, y >> 3, z >> 3) != t and (x, y, z) in at:
                        n += 1
        shell.append(n)
    got_own, got_shell = S.tile_entries(table)
    assert got_own.tolist() == own and got_shell.tolist() == shell
    span = S.tile_span(table, xyz)
    for t in order:
        first = min(tiles[t])
        for i in tiles[t]:
            assert span[i] == np.abs(xyz[i].astype(np.float64) - xyz[first].astype(np.float64)).max()
    assert max(own) > 64 and max(shell) > 128 and max(per27) >= 6   # the brute force saw the cases the predicates are for


# ---------------------------------------------------------------- svgs_supervoxels: which path each scene reaches
def test_block_1p1(oracle):
    """block_1p1 (measured): m1 3 110 seeds, 3 110 voxels labelled of 4 096; labels_per_tile 293 (m0) / 468 (m1); labels_per_256 232 (m0) /
    239 (m1); labels_per_27 24 (m0) / 27 (m1)."""
    for mode in (0, 1):
        s = _scene(oracle, "block_1p1", mode)
        assert _rounds(s["kw"]) == 1   # m1: `for (it = 1; it < depth; ++it)` never runs; m0: one round
        lt, l256, l27 = S.labels_per_tile(s["T"], s["vl"]).max(), S.labels_per_256(s["vl"]).max(), S.labels_per_27(s["T"], s["vl"]).max()
        _report("block_1p1", mode, seeds=s["seeds"], labelled=int((s["vl"] > 0).sum()), per_tile=lt, per_256=l256, per_27=l27)
        assert lt > VT_SLOTS
        assert l256 > VX_SLOTS
        assert l27 >= 6
    s = _scene(oracle, "block_1p1", 1)
    labelled = s["vl"][s["vl"] > 0]
    assert labelled.size == s["seeds"] == s["mx"] == np.unique(labelled).size   # the kept seeds only, one voxel each
    assert labelled.size < s["vl"].size
    assert (_scene(oracle, "block_1p1", 0)["vl"] > 0).all()                      # m0's one round reaches every voxel


def test_block_1p5(oracle):
    """block_1p5 (measured): labels_per_tile 185 (m0) / 59 (m1); labels_per_27 19 (m0) / 9 (m1); m1: 1 331 seeds, 191 supervoxels at the
    end, 4.9 % of the voxels without a label."""
    for mode in (0, 1):
        s = _scene(oracle, "block_1p5", mode)
        assert _rounds(s["kw"]) == 2
        lt, l27 = S.labels_per_tile(s["T"], s["vl"]).max(), S.labels_per_27(s["T"], s["vl"]).max()
        _report("block_1p5", mode, seeds=s["seeds"], max_label=s["mx"], per_tile=lt, per_27=l27, unlabelled=float((s["vl"] == 0).mean()))
        assert lt > VT_SLOTS
        assert l27 >= 6
    assert (_scene(oracle, "block_1p5", 1)["vl"] == 0).any()


def test_block_2p5_origin(oracle):
    """block_2p5_origin (measured): m1 16 tiles, own + shell 720 in the eight inner ones and 144 in the eight thin ones; own voxels up to
    448 (m1) / 348 (m0), shells up to 272 (m1) / 342 (m0)."""
    for mode in (0, 1):
        s = _scene(oracle, "block_2p5_origin", mode)
        own, shell = S.tile_entries(s["T"])
        _report("block_2p5_origin", mode, tiles=own.size, own=own.max(), shell=shell.max(), entries_max=(own + shell).max(),
                entries_min=(own + shell).min())
        assert own.max() > 64        # the `v += 64` loops of every tile kernel
        assert shell.max() > 128     # the third staging loop
        if mode == 1:                # k_pclt_normals: staged and not staged, in one run
            assert (own + shell).max() > VTN_CAP and (own + shell).min() <= VTN_CAP
        assert (s["vl"] > 0).any()
    xyz = _scene(oracle, "block_2p5_origin", 1)["xyz"]
    assert (xyz.min(axis=0) < -0.5).all() and (xyz.max(axis=0) > 0.5).all()   # the viewpoint (0, 0, 0) lies inside the cloud


def test_line_3000(oracle):
    """line_3000 (measured): 1 201 supervoxels (m0), 1 201 seeds and max_label 1 200 (m1); a tile holds at most 9 (m0) / 6 (m1) voxels."""
    for mode in (0, 1):
        s = _scene(oracle, "line_3000", mode)
        own, shell = S.tile_entries(s["T"])
        _report("line_3000", mode, seeds=s["seeds"], max_label=s["mx"], own=own.max(), entries=(own + shell).max())
        assert 1100 <= s["seeds"] <= 1300
        assert own.max() <= 9
        m = s["lab"] > 0
        x = np.bincount(s["lab"][m], s["xyz"][m, 0].astype(np.float64)) / np.maximum(np.bincount(s["lab"][m]), 1)
        present = np.unique(s["lab"][m])
        assert present.size > 900 and (np.diff(x[present]) > 0).all()   # the labels rise along the line


def test_big_voxels(oracle):
    """big_voxels (measured): tile_span 39.5 m (m0) / 36.3 m (m1) on voxels that end with a label."""
    for mode in (0, 1):
        s = _scene(oracle, "big_voxels", mode)
        span = S.tile_span(s["T"], s["xyz"])
        _report("big_voxels", mode, span=float(span[s["vl"] > 0].max()))
        assert span[s["vl"] > 0].max() >= 32.0 + 1.0   # 2^21 / 65 536 m, and a metre for the centroid's float rounding


def test_all_rejected(oracle):
    """all_rejected (measured): m1 no seed kept; m0 392 supervoxels."""
    s = _scene(oracle, "all_rejected", 1)
    assert s["seeds"] == 0 and s["mx"] == 0 and (s["lab"] == 0).all()
    s0 = _scene(oracle, "all_rejected", 0)
    _report("all_rejected", 0, max_label=s0["mx"])
    assert 380 <= s0["mx"] <= 400


def test_clutter_and_sheet(oracle):
    """clutter_and_sheet (measured): m1 16 seeds kept, all on the sheet; 30.7 % of the points without a label."""
    s = _scene(oracle, "clutter_and_sheet", 1)
    x = s["xyz"].astype(np.float64)
    on_sheet = (np.abs(x[:, 2] - 10.05) < 0.05) & (x[:, 0] > 8.0) & (x[:, 0] < 11.0) & (x[:, 1] > 8.0) & (x[:, 1] < 11.0)
    near = (np.abs(x[:, 2] - 10.05) < 1.0) & (x[:, 0] > 7.0) & (x[:, 0] < 12.0) & (x[:, 1] > 7.0) & (x[:, 1] < 12.0)   # within a seed_size
    _report("clutter_and_sheet", 1, seeds=s["seeds"], unlabelled=float((s["lab"] == 0).mean()))
    assert s["seeds"] == 16 == s["mx"]
    assert on_sheet.sum() >= 900 and (s["lab"][~near] == 0).all() and (s["lab"][on_sheet] > 0).all()   # only the sheet's seeds were kept
    assert 0.25 < (s["lab"] == 0).mean() < 0.40
    assert _scene(oracle, "clutter_and_sheet", 0)["mx"] > 300   # without rejection the clutter makes supervoxels


@pytest.mark.parametrize("name", list(S.TINY))
def test_tiny(oracle, name):
    for mode in (0, 1):
        s = _scene(oracle, "tiny_" + name, mode)
        assert s["T"]["key"].shape[0] == S.TINY[name][1]
        assert s["mx"] >= 1 and (s["lab"] > 0).any()


def test_the_two_modes_differ(oracle):
    """vccs_mode 0 and 1 are different algorithms on different lattices: a scene that both label must not come out the same."""
    a, b = _scene(oracle, "block_2p5_origin", 0), _scene(oracle, "block_2p5_origin", 1)
    assert a["T"]["key"].shape[0] != b["T"]["key"].shape[0] and (a["lab"] != b["lab"]).mean() > 0.05


# ---------------------------------------------------------------- svgs_segment on a caller's labels
SV_PARAMS = dict(voxel_size=0.05, seed_size=0.25, graph_size=0.5)


def _rows(ref):
    off, idx = ref.lists("adjacency")
    return off, idx, np.diff(off)


@pytest.mark.parametrize("size", S.HUB_SIZES + (S.SV_ROW + 1,))
def test_hub_row_is_full(oracle, size):
    """The oracle's largest adjacency row is the hub's and holds all S supervoxels (measured second largest: 22, 23, 41, 42, 158, 158)."""
    xyz, lab, mx = S.hub_and_shell(size)
    assert xyz.shape[0] == 4 * size <= 4096 + 4
    ref = oracle.run_svgs_from_labels(xyz, lab, mx, oracle.svgs_params(**SV_PARAMS))
    off, idx, rows = _rows(ref)
    assert ref.V == size and rows.max() == size and rows.argmax() == 0
    assert np.sort(rows)[-2] <= 64 or size >= 512   # only the hub's row leaves the 64-entry network below S = 512
    assert idx[off[0]] == 0                         # d2 = 0 < r2: the supervoxel itself comes first


def test_hub_edges(oracle):
    """hub_edges on the oracle: exact centroids one float step inside, on and outside graph_size; the twins tie on d2."""
    xyz, lab, mx, ids = S.hub_edges()
    ref = oracle.run_svgs_from_labels(xyz, lab, mx, oracle.svgs_params(**SV_PARAMS))
    off, idx, rows = _rows(ref)
    c = ref.nodes()["centroid"]
    r2 = np.float32(0.5 * 0.5)
    hub = c[ids["hub"]]
    assert np.array_equal(hub, np.array(S.EDGE_HUB, dtype=np.float32)) and (hub < 0).all()
    x_on = np.float32(S.EDGE_HUB[0] + 0.5)
    want = {"inside": np.nextafter(x_on, np.float32(-10)), "on": x_on, "outside": np.nextafter(x_on, np.float32(10))}
    d2 = {}
    for k, x in want.items():
        assert np.array_equal(c[ids[k]], np.array([x, S.EDGE_HUB[1], S.EDGE_HUB[2]], dtype=np.float32)), k
        t = hub - c[ids[k]]
        d2[k] = np.float32(np.float32(t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    assert d2["inside"] < r2 == d2["on"] < d2["outside"]   # one step of the x coordinate (2^-22 at 3.5) to either side of d2 == r2
    assert r2 - d2["inside"] < 1e-6 and d2["outside"] - r2 < 1e-6
    row = idx[off[0]:off[1]].tolist()
    assert ids["inside"] in row and ids["on"] not in row and ids["outside"] not in row
    assert row[-1] == ids["inside"]                       # the farthest entry of the row
    assert rows.max() == rows[0] == 129 and ref.V == 131  # padded to 256 entries
    a, b = ids["twins"]
    assert np.array_equal(c[a].view(np.uint32), c[b].view(np.uint32))
    both = [r for r in range(ref.V) if a in idx[off[r]:off[r + 1]] and b in idx[off[r]:off[r + 1]]]
    assert len(both) > 10 and 0 in both
    for r in both:                                        # a tie on d2: the lower id first, next to each other
        lst = idx[off[r]:off[r + 1]].tolist()
        assert lst.index(b) == lst.index(a) + 1, r
    assert idx[off[a]:off[a] + 2].tolist() == [a, b] and idx[off[b]:off[b] + 2].tolist() == [a, b]   # d2 = 0 twice


@pytest.mark.parametrize("name", list(S.labellings_40()))
def test_labellings(oracle, name):
    xyz, lab, mx, V, unlabelled = S.labellings_40()[name]
    ref = oracle.run_svgs_from_labels(xyz, lab, mx, oracle.svgs_params(**SV_PARAMS))
    pl, _ = ref.labels()
    assert ref.V == V and int((pl < 0).sum()) == unlabelled
    if V == 0:
        assert ref.clusters_num == 0 and (pl == -1).all()
    else:
        assert ref.clusters_num > 0
        keep = (lab > 0) & (lab < mx)
        assert np.array_equal(pl >= 0, keep)   # SVGS keeps every cluster: a point is labelled iff its supervoxel exists


def test_non_finite_points_belong_to_no_supervoxel(oracle):
    """include/vgs.h: a point with a non-finite coordinate belongs to no supervoxel, whatever label the caller gave it.  The oracle on the
    NaN labelling equals the oracle on the same cloud with those points labelled 0 (before the rule it gathered the NaN into the centroid
    and crashed on the cell index made from it; oracle/selftest.cpp runs the same scene under the sanitizers)."""
    xyz, lab, mx, bad = S.nan_labelling()
    assert bad.sum() == 10 and np.unique(lab[bad]).size == 10 and np.isnan(xyz[bad, 1]).all()
    p = oracle.svgs_params(**SV_PARAMS)
    a = oracle.run_svgs_from_labels(xyz, lab, mx, p)
    lab0 = np.where(bad, 0, lab).astype(np.int32)
    b = oracle.run_svgs_from_labels(xyz, lab0, mx, p)
    assert a.V == b.V == 40 and a.clusters_num == b.clusters_num
    assert np.array_equal(a.labels()[0], b.labels()[0]) and (a.labels()[0][bad] == -1).all() and (a.labels()[0][~bad] >= 0).all()
    for which in ("sv_points", "adjacency", "connect_final"):
        (ao, ai), (bo, bi) = a.lists(which), b.lists(which)
        assert np.array_equal(ao, bo) and np.array_equal(ai, bi), which
    na, nb = a.nodes(), b.nodes()
    assert np.isfinite(na["centroid"]).all()
    for k in na:
        assert np.array_equal(na[k].view(np.uint8), nb[k].view(np.uint8)), k
