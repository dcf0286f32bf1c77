"""The frames of tests/sequence_frames.py are what they claim (CPU oracle only): sizes, octree depth, voxel-key layout, used voxels and
kept segments of every frame as the table in sequence_frames.EXPECT states them, so a frame cannot silently stop reaching its case."""
import numpy as np
import pytest

import sequence_frames as sf


@pytest.fixture(scope="module")
def refs(oracle):
    return {name: oracle.run_vgs(sf.cloud(name), oracle.vgs_params(**sf.PARAMS[name])) for name in sf.EXPECT}


@pytest.mark.parametrize("name", list(sf.EXPECT))
def test_frame_table(refs, name):
    n, v, depth, layout, used, kept = sf.EXPECT[name]
    xyz, r = sf.cloud(name), refs[name]
    assert xyz.dtype == np.float32 and xyz.shape == (n, 3)
    got = dict(V=r.V, depth=r.depth, used=r.used_nodes, kept=r.kept_clusters)
    for key, want in (("V", v), ("depth", depth), ("used", used), ("kept", kept)):
        if want is not None:
            assert got[key] == want, (name, key, got)
    if layout is not None:
        assert sf.key_layout(r.depth, n) == layout


def test_frames_reach_their_cases(refs):
    # the three key widths, each from the same 6000 points
    assert [sf.key_layout(refs[k].depth, sf.cloud(k).shape[0]) for k in ("G", "D", "E")] == ["u32", "u64-packed", "u64"]
    g = sf.cloud("G")
    for k in ("D", "E"):
        assert np.array_equal(sf.cloud(k)[:6000], g)                       # the far points come last: the box grows late
        assert np.abs(sf.cloud(k)[6000:]).max() >= 400.0
        assert refs[k].kept_clusters == refs["G"].kept_clusters            # two lone points more, the same segments
    # no used voxel, no voxel, no point
    assert refs["F"].V > 0 and refs["F"].used_nodes == 0 and (refs["F"].labels()[0] == -1).all()
    assert refs["X"].n_finite == 0 and refs["X"].V == 0 and not np.isfinite(sf.cloud("X")).all(axis=1).any()
    assert (refs["X"].labels()[0] == -1).all() and refs["X"].labels()[0].size == 100
    assert sf.cloud("Z").shape == (0, 3) and refs["Z"].V == 0
    assert sf.cloud("T").shape == (5, 3) and refs["T"].V > 0
    # neighbours in the sequences differ in size -- or, where both hold 20000 points (C then A), in their labels -- so a copy out of
    # the wrong buffer cannot pass
    for order in ("AEHFAZDXCTA", "AHEFZCA"):
        for a, b in zip(order, order[1:]):
            if sf.cloud(a).shape[0] == sf.cloud(b).shape[0]:
                assert (a, b) == ("C", "A") and (refs[a].labels()[0] != refs[b].labels()[0]).mean() > 0.5, (order, a, b)
    # used frames really segment: labels of both signs
    for k in ("A", "C", "G", "H"):
        pl = refs[k].labels()[0]
        assert (pl >= 0).any() and (pl == -1).any() and pl.max() == refs[k].kept_clusters - 1


def test_padded_rows():
    a = sf.cloud("H")
    b = sf.padded(a)
    assert b.shape == (3000, 4) and b.dtype == np.float32 and b.flags["C_CONTIGUOUS"] and np.array_equal(b[:, :3], a)


def test_svgs_frames_keep_segments(oracle):
    """The first two clouds of the SVGS sequence keep at least 2 segments each (oracle: the PCL-order supervoxels the engine's default
    vccs_mode 1 restates, then the graph stages): 74 and 2 at these sizes."""
    p = oracle.svgs_params()
    kept = {}
    for name in ("urban", "pc"):
        xyz = sf.svgs_cloud(name)
        lab, mx = oracle.vccs_pcl(xyz, p)
        kept[name] = oracle.run_svgs_from_labels(xyz, lab, mx, p).kept_clusters
    assert kept == {"urban": 74, "pc": 2}, kept
    sizes = [sf.svgs_cloud(k).shape[0] for k in ("urban", "pc")]
    assert sizes == [60_000, 20_000]
