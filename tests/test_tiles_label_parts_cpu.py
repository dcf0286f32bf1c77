"""CPU tests of the host fold of the connected parts of a point labelling across the ranks of the tiled driver
(vgs_tiles_fold_label_parts, include/vgs_tiles.h; tiles_native.fold_label_parts) against a short union-find in Python, and of the front
end's refusals (examples/vgs_tiles_run.cpp), which come before any GPU call.

The records of a rank: its local parts (label, points, nodes, code of the first node), its band records (code, label, local part) and
its links (own local part, rank, part).  The fold unites along the links and along equal (code, label) keys of different ranks' band
records; a key with m records is one node, so m - 1 comes off the node count; the parts are numbered by (label ascending, first code
descending); label_largest takes the lowest id on a tie."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgs-svgs-segmentation_amd", "csrc")
EXE = os.path.join(ROOT, "examples", "vgs_tiles_run")
E_ARG = 1


@pytest.fixture(scope="module")
def tn(vgs):
    from vgs_svgs_segmentation_amd import tiles_native
    tiles_native.lib()
    return tiles_native


def rank(parts=(), band=(), links=()):
    """parts: (label, points, nodes, code); band: (code, label, part); links: (own, rank, part)"""
    def col(rows, i, dt):
        return np.array([r[i] for r in rows], dtype=dt)
    return dict(part_label=col(parts, 0, np.int32), part_points=col(parts, 1, np.int64), part_nodes=col(parts, 2, np.int32),
                part_first_code=col(parts, 3, np.uint64), band_code=col(band, 0, np.uint64), band_label=col(band, 1, np.int32),
                band_part=col(band, 2, np.int32), link_own=col(links, 0, np.int32), link_rank=col(links, 1, np.int32), link_part=col(links, 2, np.int32))


def ref_fold(records, K):
    """the twenty-line restatement"""
    ids = [(r, p) for r, R in enumerate(records) for p in range(len(R["part_label"]))]
    parent = {x: x for x in ids}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    for r, R in enumerate(records):
        for o, s, p in zip(R["link_own"], R["link_rank"], R["link_part"]):
            unite((r, int(o)), (int(s), int(p)))
    seen, surplus = {}, {x: 0 for x in ids}
    for r, R in enumerate(records):
        for c, l, p in zip(R["band_code"], R["band_label"], R["band_part"]):
            if (int(c), int(l)) in seen:
                unite(seen[(int(c), int(l))], (r, int(p)))
                surplus[(r, int(p))] += 1
            else:
                seen[(int(c), int(l))] = (r, int(p))
    rows = {}
    for (r, p) in ids:
        R = records[r]
        row = rows.setdefault(find((r, p)), [int(R["part_label"][p]), 0, 0, 0])
        row[1] += int(R["part_points"][p]); row[2] += int(R["part_nodes"][p]) - surplus[(r, p)]; row[3] = max(row[3], int(R["part_first_code"][p]))
    order = sorted(rows, key=lambda x: (rows[x][0], -rows[x][3]))
    gid = {x: g for g, x in enumerate(order)}
    tab = [rows[x] for x in order]
    first = [sum(1 for t in tab if t[0] < k) for k in range(K + 1)]
    largest = []
    for k in range(K):
        mine = [(-t[1], g) for g, t in enumerate(tab) if t[0] == k]
        largest.append(min(mine)[1] if mine else -1)
    return dict(part_label=[t[0] for t in tab], part_points=[t[1] for t in tab], part_nodes=[t[2] for t in tab], part_first_code=[t[3] for t in tab],
                label_first=first, label_largest=largest, n_parts=len(tab),
                map=[[gid[find((r, p))] for p in range(len(R["part_label"]))] for r, R in enumerate(records)])


def check(tn, records, K):
    got, want = tn.fold_label_parts(records, K), ref_fold(records, K)
    assert got["n_parts"] == want["n_parts"]
    for name in ("part_label", "part_points", "part_nodes", "part_first_code", "label_first", "label_largest"):
        assert got[name].tolist() == want[name], name
    assert [m.tolist() for m in got["map"]] == want["map"]
    return got


def test_empty_ranks_and_k0(tn):
    g = check(tn, [rank(), rank(), rank()], 0)
    assert g["n_parts"] == 0 and g["label_first"].tolist() == [0]
    g = check(tn, [rank(), rank([(1, 5, 2, 40)]), rank()], 3)
    assert g["label_first"].tolist() == [0, 0, 1, 1] and g["label_largest"].tolist() == [-1, 0, -1]


def test_link_seen_from_both_sides(tn):
    a = rank([(0, 10, 3, 90)], [(90, 0, 0)], [(0, 1, 0)])
    b = rank([(0, 7, 2, 80)], [(80, 0, 0)], [(0, 0, 0)])
    g = check(tn, [a, b], 1)
    assert g["n_parts"] == 1 and g["part_points"].tolist() == [17] and g["part_nodes"].tolist() == [5] and g["part_first_code"].tolist() == [90]


def test_shared_key_under_two_labels(tn):
    """the voxel 50 holds points of both ranks: under label 0 on both (one node), under label 1 on rank 0 and label 2 on rank 1 (apart)"""
    a = rank([(0, 4, 1, 50), (1, 3, 1, 50)], [(50, 0, 0), (50, 1, 1)])
    b = rank([(0, 5, 1, 50), (2, 2, 1, 50)], [(50, 0, 0), (50, 2, 1)])
    g = check(tn, [a, b], 3)
    assert g["part_label"].tolist() == [0, 1, 2] and g["part_nodes"].tolist() == [1, 1, 1] and g["part_points"].tolist() == [9, 3, 2]


def test_key_shared_by_four_ranks(tn):
    recs = [rank([(0, r + 1, 2, 70)], [(70, 0, 0)]) for r in range(4)]
    g = check(tn, recs, 1)
    assert g["n_parts"] == 1 and g["part_nodes"].tolist() == [4 * 2 - 3] and g["part_points"].tolist() == [10]


def test_transitive_chain_and_numbering_by_code(tn):
    """0 - 1 - 3 through links, ranks 0 and 3 never meet; rank 2's part of the same label has the larger code and so the lower id; equal
    point counts: label_largest takes the lower id"""
    recs = [rank([(1, 5, 2, 30)], [(30, 1, 0)], [(0, 1, 0)]), rank([(1, 3, 1, 20)], [(20, 1, 0)], [(0, 3, 0)]),
            rank([(1, 10, 4, 99)], [(99, 1, 0)]), rank([(1, 2, 1, 10)], [(10, 1, 0)])]
    g = check(tn, recs, 2)
    assert g["part_first_code"].tolist() == [99, 30] and g["part_points"].tolist() == [10, 10] and g["label_largest"].tolist() == [-1, 0]
    assert [m.tolist() for m in g["map"]] == [[1], [1], [0], [1]]


def _random_case(rng, world, K):
    codes = rng.permutation(10_000)[:200] + 1
    recs, n_parts = [], []
    for r in range(world):
        np_ = int(rng.integers(0, 12))
        parts = [(int(rng.integers(0, K)), int(rng.integers(1, 50)), int(rng.integers(1, 9)), int(rng.choice(codes))) for _ in range(np_)]
        band = {}
        for p, row in enumerate(parts):
            for c in rng.choice(codes[:40], size=int(rng.integers(0, 4)), replace=False):
                band.setdefault((int(c), row[0]), p)   # (a rank publishes a key once)
        recs.append([parts, [(c, l, p) for (c, l), p in band.items()], []])
        n_parts.append(np_)
    for r in range(world):
        for _ in range(int(rng.integers(0, 6))):
            s = int(rng.integers(0, world))
            if s == r or not n_parts[r] or not n_parts[s]:
                continue
            o = int(rng.integers(0, n_parts[r]))
            same = [p for p, row in enumerate(recs[s][0]) if row[0] == recs[r][0][o][0]]
            if same:
                recs[r][2].append((o, s, int(rng.choice(same))))
    return [rank(*x) for x in recs]


@pytest.mark.parametrize("seed", range(8))
def test_random_cases(tn, seed):
    rng = np.random.default_rng(seed)
    check(tn, _random_case(rng, int(rng.integers(1, 6)), int(rng.integers(1, 5))), 5)


def test_order_of_a_ranks_records_does_not_matter(tn):
    rng = np.random.default_rng(42)
    recs = _random_case(rng, 4, 3)
    base = tn.fold_label_parts(recs, 3)
    shuffled = []
    for R in recs:
        pb, pl = rng.permutation(len(R["band_code"])), rng.permutation(len(R["link_own"]))
        S = dict(R)
        for name in ("band_code", "band_label", "band_part"):
            S[name] = R[name][pb]
        for name in ("link_own", "link_rank", "link_part"):
            S[name] = R[name][pl]
        shuffled.append(S)
    got = tn.fold_label_parts(shuffled, 3)
    for name in ("part_label", "part_points", "part_nodes", "part_first_code", "label_first", "label_largest"):
        assert got[name].tobytes() == base[name].tobytes(), name
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got["map"], base["map"]))


@pytest.mark.parametrize("records,K", [
    ([rank([(2, 1, 1, 5)])], 2),                                                     # a label outside 0 .. K-1
    ([rank([(-1, 1, 1, 5)])], 2),
    ([rank([(0, 1, 1, 5)], links=[(0, 1, 3)]), rank([(0, 1, 1, 4)])], 1),            # a link naming a part that does not exist
    ([rank([(0, 1, 1, 5)], links=[(1, 1, 0)]), rank([(0, 1, 1, 4)])], 1),
    ([rank([(0, 1, 1, 5)], links=[(0, 2, 0)]), rank([(0, 1, 1, 4)])], 1),            # ... a rank that does not exist
    ([rank([(0, 1, 1, 5)], links=[(0, 1, 0)]), rank([(1, 1, 1, 4)])], 2),            # a link between different labels
    ([rank([(0, 1, 1, 5)], band=[(5, 0, 1)])], 1),                                   # a band record naming a part that does not exist
])
def test_refusals(tn, records, K):
    with pytest.raises(tn.VgsError) as e:
        tn.fold_label_parts(records, K)
    assert e.value.status == E_ARG


def test_null_arguments(tn):
    L = tn.lib()
    off = np.zeros(2, dtype=np.int64)
    p = off.ctypes.data_as(C.c_void_p)
    assert L.vgs_tiles_fold_label_parts(0, 0, p, *([None] * 4), p, *([None] * 3), p, *([None] * 3), *([None] * 8)) == E_ARG
    assert L.vgs_tiles_fold_label_parts(1, -1, p, *([None] * 4), p, *([None] * 3), p, *([None] * 3), *([None] * 8)) == E_ARG
    assert L.vgs_tiles_fold_label_parts(1, 0, p, *([None] * 4), p, *([None] * 3), p, *([None] * 3), *([None] * 8)) == 0


# ---------------------------------------------------------------- the front end's refusals, before any GPU call
def _run(tmp_path, opts):
    subprocess.check_call(["make", "-C", CSRC, "-s", "example"])
    return subprocess.run([EXE, "--emulate", "2x1", *opts, str(tmp_path / "t")], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("opts,word", [(["--refined-components", "a.csv"], "need --refine"),
                                       (["--component-ids"], "--component-ids needs --refined-components or --class-components"),
                                       (["--class-components", "b.csv"], "--class-components needs --classes"),
                                       (["--class-components", "b.csv", "--classes", "0"], "--classes must be in 1 .. 1024"),
                                       (["--refine", "--refined-components", "a.csv", "--class-components", "b.csv", "--classes", "4", "--component-ids"],
                                        "--component-ids serves one table")])
def test_component_options_are_refused_before_any_gpu_call(tmp_path, opts, word):
    p = _run(tmp_path, opts)
    assert p.returncode == 2 and word in p.stderr and "usage:" in p.stderr, (p.returncode, p.stderr)
    assert "--refined-components" in p.stderr and "--class-components" in p.stderr and "--component-ids" in p.stderr
    assert not os.listdir(tmp_path)


def test_missing_class_file_is_a_usage_error(tmp_path):
    np.zeros((10, 3), np.float32).tofile(str(tmp_path / "t.0.f32"))
    np.zeros((10, 3), np.float32).tofile(str(tmp_path / "t.1.f32"))
    before = sorted(os.listdir(tmp_path))
    p = _run(tmp_path, ["--class-components", str(tmp_path / "b.csv"), "--classes", "4"])
    assert p.returncode == 2 and "classes.i32" in p.stderr, (p.returncode, p.stderr)
    assert sorted(os.listdir(tmp_path)) == before
