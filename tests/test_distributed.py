"""world_size-2 gloo tests of the multi-process path bench.py uses: sample
sharding without a data-path collective, barrier + MAX-over-ranks timing."""
import importlib
import os
import socket

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n_total, out):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    shard = importlib.import_module("sr-for-cfd_amd.shard")
    bench = importlib.import_module("bench")
    lo, hi = shard.shard_range(n_total, rank, world)
    # every rank builds its own synthetic batch (weak scaling), seeded by rank like bench.py
    lr = {c: (0.1 * (i + 1), 0.2 + 0.1 * i) for i, c in enumerate("uvp")}
    x, ain, aout = bench.build_inputs(4, seed=rank, stats_lr=lr, stats_hr=lr)
    dist.barrier()
    t = shard.max_over_ranks(0.5 + rank)  # rank 1 is "slower"
    gathered = [None] * world
    dist.all_gather_object(gathered, (lo, hi, float(x.sum())))
    if rank == 0:
        out.put((t, gathered, x.shape, ain.tolist()))
    dist.destroy_process_group()


def test_two_rank_sharding_and_timing():
    world, n_total = 2, 769
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_total, q)) for r in range(world)]
    for p in procs:
        p.start()
    t, gathered, shape, ain = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert t == 1.5  # MAX over ranks
    (lo0, hi0, s0), (lo1, hi1, s1) = gathered
    assert (lo0, hi0, lo1, hi1) == (0, 385, 385, 769)  # contiguous, disjoint, covering, sizes differ by <= 1
    assert s0 != s1  # ranks generate different synthetic batches
    assert shape == (12, 10, 10, 1)
    assert ain[0] == pytest.approx([0.1, 0.2]) and ain[4] == pytest.approx([0.2, 0.3])  # sample 3f+c carries component c's stats


def test_shard_range_properties():
    shard = importlib.import_module("sr-for-cfd_amd.shard")
    for n in (0, 1, 7, 48, 768):
        for w in (1, 2, 3, 8):
            spans = [shard.shard_range(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        shard.shard_range(10, 2, 2)
    assert shard.aggregate_throughput(256, 8, 0.001) == 256 * 8 / 0.001


def _tiled_worker(rank, world, port, out):
    import sys
    sys.path.insert(0, ROOT)
    import numpy as np
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pl = importlib.import_module("sr-for-cfd_amd.pipeline")

    class Up:  # nearest-neighbour x2 stand-in with the SRModel.predict signature; counts the samples it is given
        seen = 0

        def predict(self, x, in_affine=None, out_affine=None):
            Up.seen += x.shape[0]
            return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)

    f = np.arange(40 * 40 * 3, dtype=np.float32).reshape(40, 40, 3)
    y = pl.tiled_super_resolution(f, Up(), lr_dim=10, distributed=True)
    out.put((rank, Up.seen, bool(np.array_equal(y, np.repeat(np.repeat(f, 2, axis=0), 2, axis=1)))))
    dist.barrier()
    dist.destroy_process_group()


def test_tiled_sr_sharded_over_three_ranks():
    """BASELINE config 5 across ranks: 48 tile samples over 3 ranks (16 each), one all_gather, every rank stitches the whole field."""
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tiled_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [g[1] for g in got] == [16, 16, 16] and all(g[2] for g in got)


def _run_bench(argv, env_extra, timeout=600):
    import json
    import subprocess
    import sys
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    return p.returncode, [json.loads(ln) for ln in lines], p.stderr


def test_bench_gpus_flag_starts_that_many_ranks():
    """`python bench.py --gpus 2` with no WORLD_SIZE must itself start two ranks (children, before any GPU call) and print ONE line
    with n_gpus = 2 = the world size the process group reports.  Rank plumbing only: SRCFD_BENCH_DRYRUN."""
    rc, recs, err = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1"], {"SRCFD_BENCH_DRYRUN": "1"})
    assert rc == 0, err
    assert len(recs) == 1
    r = recs[0]
    assert r["n_gpus"] == 2 and r["world_size_reported"] == 2 and r["dry_run"] is True and r["value"] is None
    assert r["max_over_ranks"] == 2.0 and r["tile_samples_covered"] == 48
    assert r["env"] == {"SRCFD_BENCH_DRYRUN": "1"}          # every SRCFD_* variable is recorded in the line


def test_bench_eight_rank_rehearsal():
    """`bench.py --gpus 8` as the driver's 8-GPU node will run it, rehearsed with gloo and no device work: eight ranks come up,
    the 48 tile samples of config 5 shard 6 per rank, the training legs see global batch 64 (weak) and 32 samples per rank
    (strong, global batch 256), min / max over ranks are both reduced, and the outcome of a leg that fails on ONE rank is known
    on every rank (the all-or-none agreement that keeps the others out of a collective)."""
    rc, recs, err = _run_bench(["--gpus", "8", "--steps", "3", "--warmup", "1", "--full"], {"SRCFD_BENCH_DRYRUN": "1"})
    assert rc == 0, err[-2000:]
    r = recs[0]
    assert r["n_gpus"] == 8 and r["world_size_reported"] == 8 and r["fields_total"] == 8 * 256
    assert r["tile_samples_per_rank"] == [6] * 8 and r["tile_samples_covered"] == 48
    assert r["train"]["global_batch"] == 64 and r["train"]["strong"] == {"global_batch": 256, "samples_per_rank": 32}
    assert r["max_over_ranks"] == 8.0 and r["min_over_ranks"] == 1.0 and r["leg_failed_somewhere"] is False
    # capacity: what eight ranks reserve (library-side sizes, nothing allocated) against this host's memory and one GPU's 288 GB
    b = r["budget"]
    assert "error" not in b, b
    assert b["fits"] is True and 1e9 < b["per_rank_device_bytes"] < 20e9, b
    legs = b["legs"]
    assert legs["headline_bf16"]["device_workspace"] == 2 * 768 * 160000 * 2 + 16 * 768 * 128 * 4
    assert legs["headline_bf16"]["host_result"] == 768 * 160000 * 4 == b["host_pinned_bytes_rank0"]
    assert legs["parity_fp32"]["device_workspace"] == 2 * 768 * 160000 * 4        # ConvT#1's output is the largest tensor the f32 path materialises
    assert legs["tiled_f16"]["device_workspace"] == 2 * 6 * 160000 * 2 + 16 * 6 * 128 * 4
    # rank 0's own legs run behind the collective ones for any N, the other ranks wait at one barrier: the N > 1 line carries them
    assert r["cpu_baseline"]["value"] > 0 and r["cpu_baseline"]["kind"] == "port" and r["cpu_baseline"]["cores"] >= 1, r["cpu_baseline"]
    rc, recs, err = _run_bench(["--gpus", "8", "--steps", "3", "--warmup", "1", "--full"], {"SRCFD_BENCH_DRYRUN": "1", "SRCFD_BENCH_DRYRUN_FAIL_RANK": "5"})
    assert rc == 0 and recs[0]["leg_failed_somewhere"] is True


def test_bench_refuses_mismatched_world_and_diagnostic_switches():
    rc, recs, err = _run_bench(["--gpus", "4"], {"SRCFD_BENCH_DRYRUN": "1", "WORLD_SIZE": "2", "RANK": "0"})
    assert rc != 0 and not recs and "WORLD_SIZE=2" in err
    for var in ("SRCFD_TAIL_ABLATE", "SRCFD_MID_ABLATE", "SRCFD_TAIL_PROF", "SRCFD_TAIL32_ABLATE"):
        rc, recs, err = _run_bench([], {var: "1"})
        assert rc != 0 and not recs and var in err
    # A/B switches select another implementation than the shipped one: no headline under them either
    for var, val in (("SRCFD_ENC", "0"), ("SRCFD_MID", "0"), ("SRCFD_MID", "1"), ("SRCFD_MID", "2"), ("SRCFD_DENSE1", "0"), ("SRCFD_NO_ENC32", "1"), ("SRCFD_NO_DENSE_SKINNY", "1"),
                     ("SRCFD_TAIL", "s"), ("SRCFD_TAIL_SEG", "5"), ("SRCFD_LIB", "/nonexistent/libsrcfd.so")):
        rc, recs, err = _run_bench([], {var: val})
        assert rc != 0 and not recs and var in err, (var, err[-300:])
    rc, recs, err = _run_bench(["--gpus", "2"], {"SRCFD_BENCH_DRYRUN": "1", "SRCFD_ENC": "1", "SRCFD_MID": "3"})   # the default value of a switch is no switch
    assert rc == 0 and len(recs) == 1


def test_bench_refuses_a_stale_traffic_file(tmp_path, monkeypatch):
    """roofline.traffic comes from committed PMC passes (bench.py cannot profile itself): a file is used only while the kernel
    sources it was taken on are the ones in the tree."""
    import json
    import sys
    sys.path.insert(0, ROOT)
    import bench
    name = "pmc_traffic_tail.json"
    good = {"source": "x", "config": {"fields": 256, "precision": "bf16", "out_dtype": "f32"}, "hbm_bytes_per_launch": 123,
            "kernel_source_stamp": bench.kernel_source_stamp(name)}
    (tmp_path / "profiles").mkdir()
    (tmp_path / "sr-for-cfd_amd").symlink_to(os.path.join(ROOT, "sr-for-cfd_amd"))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    (tmp_path / "profiles" / name).write_text(json.dumps(good))
    assert bench.measured_traffic(256, "bf16", "f32") == (123, "x")
    assert bench.measured_traffic(128, "bf16", "f32") == (None, None)                 # another configuration
    (tmp_path / "profiles" / name).write_text(json.dumps(dict(good, kernel_source_stamp="0" * 16)))
    t, why = bench.measured_traffic(256, "bf16", "f32")
    assert t is None and "stale" in why
    (tmp_path / "profiles" / name).write_text(json.dumps({k: v for k, v in good.items() if k != "kernel_source_stamp"}))
    assert bench.measured_traffic(256, "bf16", "f32")[0] is None                      # an unstamped file counts as stale


@pytest.mark.gpu
def test_bench_two_ranks_share_one_gpu():
    """The full rank path of bench.py (`--gpus 2` -> two child ranks, barrier, MAX over ranks, aggregate) on ONE GPU with the
    gloo backend standing in for RCCL; 8 fields per rank.  n_gpus and the aggregate must reflect both ranks."""
    rc, recs, err = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--fields", "16", "--full"],
                               {"SRCFD_BENCH_BACKEND": "gloo", "SRCFD_BENCH_CPU_BUDGET_S": "1"}, timeout=900)
    assert rc == 0, err[-2000:]
    r = recs[0]
    assert r["n_gpus"] == 2 and r["world_size_reported"] == 2
    assert r["value"] == pytest.approx(2 * 16 / (r["ms_per_step"] * 1e-3), rel=1e-3)
    # an N > 1 line is complete: CPU stand-in, both rooflines, the float64-oracle check of both paths, the host-buffer entry
    assert r["cpu_baseline"]["value"] > 0 and r["cpu_baseline"]["gpu_rel_l2_vs_f64_oracle"]["bf16"] < 2e-2
    assert r["parity_path"]["rel_l2_vs_f64_oracle"] <= 1e-5 and r["host_io"] is not None and "sub_record_errors" not in r, r.get("sub_record_errors")
    assert r["parity_path_x3"]["rel_l2_vs_f64_oracle"] <= 1e-5
    best = r["fastest_path_within_1e-5"]
    assert best["precision"] in ("fp32", "fp32x3") and best["rel_l2_vs_f64_oracle"] <= 1e-5
    assert best["value"] == max(r["parity_path"]["value"], r["parity_path_x3"]["value"])
    assert r["kernels_ms_sum"] * r["kernels_ms_in_step_scale"] <= r["ms_per_step"] * 1.0001
    assert r["nonfinite"] == 0 and r["roofline"]["frac"] > 0
    assert r["parity_path"]["roofline"]["avg_launch_ms"] <= r["parity_path"]["ms_per_step"] * 1.02
    assert r["train"]["global_batch"] == 16 and r["train"]["loss_finite"]
    assert r["tiled"]["tile_samples"] == 48


@pytest.mark.gpu
def test_bench_needs_as_many_devices_as_ranks():
    import torch
    n = torch.cuda.device_count()
    rc, recs, err = _run_bench(["--gpus", str(n + 1), "--steps", "1", "--warmup", "0", "--no-extras", "--no-cpu-baseline"], {}, timeout=600)
    assert rc != 0 and not recs


@pytest.mark.gpu
def test_rccl_backend_two_gpus():
    """The real `nccl` (= RCCL) backend: `bench.py --gpus 2` on two GPUs -- sample-sharded inference with the scalar MAX
    reduction, and the data-parallel training step's flat-gradient all-reduce over xGMI.  Needs two visible devices: on a
    one-GPU box this is reported as SKIPPED (the N > 1 hardware runs are the driver's)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs 2 GPUs for the RCCL backend, {torch.cuda.device_count()} visible")
    rc, recs, err = _run_bench(["--gpus", "2", "--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline"], {}, timeout=900)
    assert rc == 0, err[-2000:]
    r = recs[0]
    assert r["n_gpus"] == 2 and r["world_size_reported"] == 2 and r["config"]["backend"] == "nccl"
    assert r["value"] == pytest.approx(2 * 256 / (r["ms_per_step"] * 1e-3), rel=1e-3) and r["nonfinite"] == 0
    assert r["train"]["global_batch"] == 16 and "nccl" in r["train"]["collective"] and r["train"]["loss_finite"]
