"""The frames of the cloud-sequence tests (test_gpu_sequence.py, test_sequence_frames_cpu.py): small clouds that differ in size, content,
voxel-key layout and in which early return of the stages they reach.  Pure numpy and the package's deterministic scenes; nothing here
touches a device.

EXPECT holds what the CPU oracle (oracle.run_vgs, DevMath / lean) gives for every frame -- N, V, octree depth, key layout, used voxels,
kept segments -- and test_sequence_frames_cpu.py asserts it, so a frame cannot silently stop reaching its case.  None: not pinned."""
import numpy as np

from vgs_svgs_segmentation_amd import scenes

# parameters that differ from the Task-file defaults (gpu.default_params(2, **PARAMS[name]))
PARAMS = {
    "A": {}, "G": {}, "H": {}, "D": {}, "E": {}, "Z": {}, "X": {}, "T": {},
    "C": dict(voxel_size=0.05, graph_size=0.25),
    "F": dict(voxel_size=0.08, cut_thred=0.9),
}

# frame: (N, V, depth, key layout, used, kept)
EXPECT = {
    "A": (20000, 1198, 7, "u32", 863, 51),
    "C": (20000, 1166, 7, "u32", 772, 10),
    "G": (6000, 594, 6, "u32", 263, 19),
    "H": (3000, 407, 4, "u32", 105, 9),
    "D": (6002, 596, 12, "u64-packed", 263, 19),
    "E": (6002, 596, 18, "u64", 263, 19),
    "F": (21170, 12191, 7, "u32", 0, 0),
    "Z": (0, 0, None, None, 0, 0),
    "X": (100, 0, None, None, 0, 0),
    "T": (5, None, None, None, None, None),
}

# frames whose point labels and kept count the GPU tests also compare with the oracle
ORACLE_FRAMES = ("A", "C", "D", "E", "F", "T")

_CACHE = {}


def key_layout(depth, n):
    """What the voxelize stage chooses (test_gpu_voxel_runs._key_layout): 32-bit keys while the valid bit and 3 * depth code bits fit;
    else 64-bit keys, with the point index packed below the code while it fits too, or carried by a pair sort."""
    key_bits = 3 * depth + 1
    idx_bits = 1
    while idx_bits < 32 and (1 << idx_bits) < n:
        idx_bits += 1
    if key_bits <= 32:
        return "u32"
    return "u64-packed" if key_bits + idx_bits <= 64 else "u64"


def _with_far_points(xyz, far):
    """The far points come LAST: the octree box grows late, behind every other point."""
    return np.concatenate([xyz, np.asarray(far, dtype=np.float32)]).astype(np.float32)


def _make(name):
    if name == "A":
        return scenes.town_scene(20_000)
    if name == "C":
        return scenes.pc_scene(20_000)
    if name == "G":
        return scenes.town_scene(6_000)
    if name == "H":
        return scenes.town_scene(3_000)
    if name == "D":
        return _with_far_points(cloud("G"), [(400.0, 0.0, 0.0), (0.0, -400.0, 1.0)])
    if name == "E":
        return _with_far_points(cloud("G"), [(12000.0, 0.0, 0.0), (0.0, 12000.0, 1.0)])
    if name == "F":   # no voxel reaches points_min (test_gpu_edge.test_no_voxel_with_enough_points)
        return scenes.urban_scene(21_170, seed=206792296)
    if name == "Z":
        return np.zeros((0, 3), np.float32)
    if name == "X":   # only non-finite points (test_gpu_edge.test_only_non_finite_points)
        xyz = np.full((100, 3), np.nan, np.float32)
        xyz[::3, 1] = np.inf
        return xyz
    if name == "T":   # test_gpu_edge.test_tiny_clouds, n = 5
        rng = np.random.default_rng(5)
        return (rng.standard_normal((5, 3)) * 0.05 + np.array([2.0, -1.0, 0.5])).astype(np.float32)
    raise KeyError(name)


def cloud(name):
    """The (N, 3) float32 cloud of a frame; made once, read-only."""
    if name not in _CACHE:
        xyz = np.ascontiguousarray(_make(name), dtype=np.float32)
        xyz.setflags(write=False)
        _CACHE[name] = xyz
    return _CACHE[name]


def padded(xyz):
    """The same cloud as (N, 4) rows (pcl::PointXYZ: 16-byte points); the fourth float is never read."""
    return np.concatenate([xyz, np.ones((xyz.shape[0], 1), np.float32)], axis=1)


# SVGS (method 3) sequence: two clouds for the engine's own supervoxels, a third for a caller's labelling
SVGS_N = {"urban": 60_000, "pc": 20_000, "town": 30_000}


def svgs_cloud(name):
    key = "svgs_" + name
    if key not in _CACHE:
        xyz = {"urban": scenes.urban_scene, "pc": scenes.pc_scene, "town": scenes.town_scene}[name](SVGS_N[name])
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        xyz.setflags(write=False)
        _CACHE[key] = xyz
    return _CACHE[key]
