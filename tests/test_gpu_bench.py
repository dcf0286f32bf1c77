"""bench.py end to end on an MI355X at reduced sizes: the plain single-GPU line, the --full one with its host-to-host leg, and the N > 1 branch
(TiledSegmenter + process group) with two ranks sharing the one GPU over gloo (VGS_BENCH_BACKEND / VGS_BENCH_SINGLE_DEVICE:
a 1-GPU box cannot run RCCL with two ranks)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_single_gpu_line(gpu):
    out = _run(["--points", "400000", "--steps", "3", "--warmup", "1", "--full"])
    assert out["n_gpus"] == 1 and out["value"] > 0 and out["unit"] == "points/s" and out["dtype"] == "f32"
    assert set(out["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"}
    h = out["host_to_host"]
    assert h["labels_equal_device_resident_run"] is True and h["value"] > 0 and h["latency_ms_median"] > 0
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0 and cb["cpu_lean"]["value"] >= cb["value"]
    assert cb["cpu_lean_all_cores"]["cores"] >= 1 and cb["cpu_lean_all_cores"]["value"] > 0
    assert out["stage_ms"]["labels"] > 0.0
    assert out["clusters_ms"]["clusters"] == out["config"]["segments"]


def test_plain_line_is_the_headline_alone(gpu):
    """Without --full the line carries the timed steps' figures and nothing that takes runs of its own."""
    out = _run(["--points", "400000", "--steps", "3", "--warmup", "1"])
    assert out["n_gpus"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert out["stage_ms"]["labels"] > 0.0 and out["roofline"]["kernel_ms"] > 0.0
    assert not {"host_to_host", "clusters_ms", "cpu_baseline"} & set(out)


def test_two_ranks_on_one_gpu(gpu):
    out = _run(["--gpus", "2", "--points", "300000", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"],
               env_extra={"VGS_BENCH_BACKEND": "gloo", "VGS_BENCH_SINGLE_DEVICE": "1"})
    assert out["n_gpus"] == 2 and out["ranks"] == 2 and out["value"] > 0 and out["scaling"] == "weak"
    assert "2x1" in out["config"]["workload"]
    # the product's driver ran (libvgs_tiles.so; its collectives through the caller's gloo group, as two ranks share the GPU)
    d = out["driver"]
    assert d["kind"].startswith("native") and len(d["per_rank"]) == 2 and d["exchange_ms"] >= 0
    assert all(r["tiles_ms"]["stages"] > 0 and r["n_boundary_records"] > 0 for r in d["per_rank"])
    twin = _run(["--gpus", "2", "--points", "300000", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--python-twin"],
                env_extra={"VGS_BENCH_BACKEND": "gloo", "VGS_BENCH_SINGLE_DEVICE": "1"})
    assert twin["driver"]["kind"].startswith("python twin")
    assert twin["config"]["voxels"] == out["config"]["voxels"]        # rank 0's tile + halo: the same cloud either way


def test_native_driver_with_a_one_rank_rccl_communicator(gpu):
    """`--gpus 1 --native`: the path every rank of a multi-GPU run takes -- ncclGetUniqueId, ncclCommInitRank, vgs_tiles_create over
    VGS_TILES_COMM_RCCL, ncclAllGather inside vgs_tiles_run -- with the world a 1-GPU box can form."""
    out = _run(["--gpus", "1", "--native", "--points", "300000", "--steps", "2", "--warmup", "1"])
    d = out["driver"]
    assert d["kind"].startswith("native") and d["rccl_ranks"] == 1 and out["ranks"] == 1 and out["value"] > 0
    assert d["per_rank"][0]["tiles_ms"]["exchange"] > 0


def test_native_driver_costs_what_the_plain_engine_costs(gpu):
    """`--gpus 1 --native` (the path every rank of a multi-GPU run takes) against the plain single-GPU line on the same cloud: the tiled
    protocol of a rank without neighbours -- shared grid, boundary records, one exchange, label hand-back -- must stay a small part of
    a step, or the N > 1 lines would say more about the driver than about the GPUs.  Measured in round 5 at 4 M points: 7.9 % before the
    grid the driver has just replayed stopped being scanned again by the voxelize stage (vgs_set_grid_covering), 5.9 % after.  At the
    bench's own 10 M points the native step was 7.54 ms against the plain 6.59 (14 %) until the end of the round, when three things a tile
    did for nothing went: its unions waited for ownership behind closestCheck although ownership is known from the lattice (now: first
    hooks and unions beside the hand-over kernels, as in the plain engine, -0.33 ms), every row was read for boundary records although only
    rows near a border line can have a neighbour of the other ownership (-0.16 ms), and the per-point labels were scattered twice (local
    names, then global: the first is now left to whoever asks, -0.14 ms): **6.91 against 6.57 ms, 5 %** -- grid phase 0.25 ms (the voxelize
    stage is 0.14 shorter for it), records 0.09, the exchange 0.06, labels handed back 0.16.  Host-side phases vary box to box, so the bar
    here is 12 % + 0.1 ms at 4 M points; the 3 % the review asked for is not reached.  Both lines carry the per-rank device memory in use."""
    plain = _run(["--points", "4000000", "--steps", "8", "--warmup", "3", "--no-cpu-baseline", "--no-host-to-host", "--no-clusters"])
    native = _run(["--gpus", "1", "--native", "--points", "4000000", "--steps", "8", "--warmup", "3"])
    a, b = plain["ms_per_step_median"], native["ms_per_step_median"]
    assert abs(b - a) <= 0.12 * a + 0.1, (a, b, native["driver"]["per_rank"][0]["tiles_ms"])
    r0 = native["driver"]["per_rank"][0]
    assert 0.1 < r0["hbm_in_use_gb"] < r0["hbm_total_gb"]


def test_dump_outputs_are_the_timed_labels(gpu, tmp_path):
    """--dump-outputs writes the per-point labels of the last timed step: those of a plain engine run on the same seeded cloud."""
    import numpy as np
    out = _run(["--points", "400000", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-host-to-host", "--no-clusters",
                "--dump-outputs", str(tmp_path)])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["dump_outputs"]["arrays"]["point_labels"]["dtype"] == "float32"
    dumped = np.load(tmp_path / "point_labels.npy")
    eng = gpu.Engine(gpu.default_params(2, voxel_size=0.1))
    eng.set_points(gpu.scenes.urban_scene(400000))
    eng.run()
    labels = eng.point_labels()
    eng.close()
    assert dumped.dtype == np.float32 and dumped.shape == labels.shape and np.array_equal(dumped, labels)
