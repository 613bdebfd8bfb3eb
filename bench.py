#!/usr/bin/env python3
"""Headline benchmark: batched super-resolution inference, BASELINE.json config 2.

    python bench.py --gpus N --steps K --warmup W

A step = one pass of the SR hot path over one batch of 256 synthetic fields
(256 x (10,10,3) -> (400,400,3) = 768 single-channel samples through
encoder_10 + decoder_400) per GPU, inputs resident in HBM, including the
per-channel standardise / de-standardise / NaN guard the reference does around
`predict` (PyCFD_ML_accelerated.py:841-876).  Weak scaling: every rank
processes its own 256 fields, no data-path collective.

`--gpus N` with N > 1 and no WORLD_SIZE in the environment starts the N ranks
itself as CHILD processes (`python -m torch.distributed.run --nproc-per-node N
bench.py ...`) before this process imports torch or touches a GPU, relays rank
0's JSON line and exits with the launcher's code.  Under an external
`torch.distributed.run` (WORLD_SIZE set) it is one rank; WORLD_SIZE != --gpus
is an error.  A rank exits non-zero when fewer devices than ranks are visible.

Prints ONE JSON line (rank 0).  A plain run does only what the headline needs: set-up, warm-up, the K timed steps of the
headline SR batch, and the line (metric, value, unit, higher_is_better, dtype, ms_per_step, ...).  `--full` adds every other
measurement and check, each after the headline:
  roofline      dominant kernel (tail16), HIP events on the launch stream
  cpu_baseline  torch-CPU (oneDNN) restatement timed on the host cores (N = 1)
  parity_path   the same batch through the f32 kernels (the <= 1e-5 path):
                fields/s, ms/step, its own roofline, rel-L2 vs the f64 oracle
  parity_path_x3  the same at SRCFD_PREC_FP32X3 (f32-grade: the two wide decoder
                layers as six bf16 MFMAs on exactly split operands), same fields
  fastest_path_within_1e-5  which of the two it was in this run (oracle-checked)
  train         BASELINE config 4: conv-AE training step, micro-batch 8 per
                GPU, flat-gradient all-reduce (RCCL) + Adam, samples/s
  tiled         BASELINE config 5: 40x40x3 -> 1600x1600x3 through 4x4 tiles, f16
  host_io       srcfd_predict with host buffers (PCIe + page faults included)
  env           every SRCFD_* variable seen (diagnostic switches are refused), and
                the device clocks / power before and after the headline
`--no-extras` / `--no-cpu-baseline` drop parts of what `--full` adds.

`--dump-outputs DIR` (rank 0) writes what the timed path returned in its LAST timed step, as .npy files:
  y.npy               DUMP_SAMPLES predicted single-channel samples (n, 400, 400, 1), as float32 whatever --out-dtype, at the
                      indices of y_sample_index.npy (a fixed, seeded sample; all of them when the batch has no more)
  y_sample_index.npy  those sample indices (float64)
The inputs depend on the arguments and the rank only (seeded), so two builds can be compared output for output.
"""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENCODER_H5 = os.path.join(GOLDEN, "vanilla_encoder10_to_400_swish_trained_upto_700_multiBC.h5")
STATS_TXT = os.path.join(GOLDEN, "standardization_stats_10to400_swish_trained_upto_700_multiBC.txt")

FIELDS = 256                      # BASELINE.json config 2
MACS_PER_SAMPLE = 140_024_128
PEAK_BF16_TFLOPS = 2500.0         # MI355X dense bf16/f16 MFMA (MI355X_MICROARCH.md)
PEAK_FP32_TFLOPS = 157.3          # f32-input MFMA
PEAK_HBM_GBS = 8000.0
DUMP_SAMPLES = 64                 # --dump-outputs: 64 f32 fields of 400 x 400 = 41 MB
PRE_WARM_MS = 120.0               # untimed steps by wall time in front of the counted warm-up of an SR leg (clock ramp; Job.timed)
REFUSED_ENV = ("SRCFD_TAIL_ABLATE", "SRCFD_MID_ABLATE", "SRCFD_TAIL_PROF", "SRCFD_TAIL32_ABLATE")   # switch work off / add syncs: never a headline
# A/B switches: each selects a complete second implementation of a stage (results stay right), but a line measured under one is
# not the shipped path: refused like the diagnostic switches (SRCFD_BENCH_ALLOW_DIAG=1 marks the line INVALID instead)
AB_ENV_OFF_WHEN_ZERO = ("SRCFD_ENC", "SRCFD_DENSE1")
AB_ENV_DEFAULT_VALUE = {"SRCFD_MID": "3"}    # workgroup shape of mid16: 3 = 4 waves x 64 pixels (shipped), 2 = 8 x 64, 1 = 8 x 32; 0 = generic GEMMs
AB_ENV_ON_WHEN_SET = ("SRCFD_NO_ENC32", "SRCFD_NO_DENSE_SKINNY", "SRCFD_NO_TAIL32", "SRCFD_NO_GEMM32_BIG", "SRCFD_NO_PAIR", "SRCFD_NO_TRIPLE")
AB_ENV_ANY_VALUE = ("SRCFD_TAIL", "SRCFD_TAIL_SEG", "SRCFD_MID_WAVES", "SRCFD_MID_ORDER", "SRCFD_GRAPH", "SRCFD_LIB", "SRCFD_TRAIN_OVERLAP", "SRCFD_TRAIN_GRAPH",
                    "SRCFD_TRAIN_FUSE", "SRCFD_TRAIN_TAIL", "SRCFD_TRAIN_ENC", "SRCFD_TRAIN_AUX_FROM")
# kernel sources whose content the committed PMC traffic files are stamped with (tools/pmc_traffic.py): a traffic figure taken
# on other kernels than the ones in this tree is not reported
TRAFFIC_SOURCES = {"pmc_traffic_tail.json": ("kernels_bf16.hip", "tail16_layout.h", "dev16.h", "kernels16.h"),
                   "pmc_traffic_fp32.json": ("kernels_tail32.hip", "kernels_gemm32.hip", "kernels_enc32.hip", "kernels_mid32.hip", "kernels.h")}


def kernel_source_stamp(name):
    """sha256 over the kernel sources a traffic file describes (missing files are skipped: the list may name future ones)."""
    import hashlib
    h = hashlib.sha256()
    for f in TRAFFIC_SOURCES[name]:
        try:
            with open(os.path.join(ROOT, "sr-for-cfd_amd", "csrc", f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
        except OSError:
            pass
    return h.hexdigest()[:16]


def srcfd_env():
    return {k: v for k, v in sorted(os.environ.items()) if k.startswith("SRCFD_")}


def non_default_switches(env):
    """SRCFD_* variables that change WHICH kernels run (diagnostic or A/B): a headline line is never reported under them."""
    bad = [k for k in env if k in REFUSED_ENV and env[k] not in ("", "0")]
    bad += [k for k in AB_ENV_OFF_WHEN_ZERO if k in env and env[k].strip() == "0"]
    bad += [k for k, dflt in AB_ENV_DEFAULT_VALUE.items() if env.get(k, "").strip() not in ("", dflt)]
    bad += [k for k in AB_ENV_ON_WHEN_SET if env.get(k, "") not in ("", "0")]
    bad += [k for k in AB_ENV_ANY_VALUE if env.get(k, "") != ""]
    return bad


def gpu_state(pci_bus_id=None):
    """Clocks / power of the device as the driver reports them ("state clocks/power mode"), read from sysfs -- plain
    file reads: a process that has initialised the GPU must not start another program on this pool (so no rocm-smi / amd-smi child).
    Read before and after the headline leg: an idle device reports its sleep clocks, which is the point -- the record shows in
    which state the leg started.  pci_bus_id: "0000:75:00.0"-style id of the HIP device; None: the first card with clock files.
    Never raises."""
    import glob
    out = {}
    try:
        cards = sorted(glob.glob("/sys/class/drm/card[0-9]*/device/pp_dpm_sclk"))
        pick = None
        for f in cards:
            dev = os.path.dirname(f)
            if pci_bus_id and os.path.basename(os.path.realpath(dev)).lower() == pci_bus_id.lower():
                pick = dev
                break
        if pick is None and cards:
            pick = os.path.dirname(cards[0])
            out["note"] = "card not matched by PCI id: first card with clock files"
        if pick is None:
            return {"error": "no /sys/class/drm/card*/device/pp_dpm_sclk"}

        def cur(name):
            try:
                for ln in open(os.path.join(pick, name)).read().splitlines():
                    if ln.rstrip().endswith("*"):
                        return ln.split(":", 1)[1].replace("*", "").strip()
            except OSError:
                return None
            return None

        def num(pattern, scale):
            for f in glob.glob(os.path.join(pick, pattern)):
                try:
                    return round(int(open(f).read().strip()) / scale, 1)
                except (OSError, ValueError):
                    pass
            return None

        out.update({"card": os.path.basename(os.path.dirname(pick)), "sclk": cur("pp_dpm_sclk"), "mclk": cur("pp_dpm_mclk"), "fclk": cur("pp_dpm_fclk"),
                    "power_W": num("hwmon/hwmon*/power1_average", 1e6) or num("hwmon/hwmon*/power1_input", 1e6),
                    "power_cap_W": num("hwmon/hwmon*/power1_cap", 1e6)})
        try:
            out["perf_level"] = open(os.path.join(pick, "power_dpm_force_performance_level")).read().strip()
        except OSError:
            pass
    except Exception as e:   # noqa: BLE001
        out["error"] = f"{type(e).__name__}: {e}"[:120]
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f16", "fp32", "fp32x3"])
    ap.add_argument("--out-dtype", default="f32", choices=["f32", "bf16", "f16"])
    ap.add_argument("--fields", type=int, default=FIELDS)
    ap.add_argument("--workload", default="sr", choices=["sr", "tiled"],
                    help="sr: BASELINE config 2 (headline); tiled: config 5 as the headline line (40x40x3 -> 1600x1600x3, f16)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement besides the headline: roofline / per-kernel times, parity paths, CPU baseline, train, tiled, host_io")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the parity_path / train / tiled / host_io sub-records")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path returned in its last timed step to DIR/<name>.npy (float32 / float64)")
    return ap.parse_args(argv)


def dump_index(n, k=DUMP_SAMPLES, seed=0):
    """The fixed, seeded sample of result indices --dump-outputs writes (sorted; all n when n <= k)."""
    import numpy as np
    if n <= k:
        return np.arange(n)
    return np.sort(np.random.default_rng(seed).choice(n, k, replace=False))


def write_outputs(out_dir, arrays):
    """--dump-outputs: one DIR/<name>.npy per array, float32 or float64 only."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        a = np.asarray(a)
        if a.dtype not in (np.float32, np.float64):
            raise TypeError(f"dump {name}: {a.dtype} is neither float32 nor float64")
        np.save(os.path.join(out_dir, name + ".npy"), a)


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(args, argv):
    """Parent side of `--gpus N`: nothing here imports torch or initialises HIP."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith('{"metric"'):
            line = ln
        else:
            print(ln, file=sys.stderr)
    if proc.returncode != 0 or line is None:
        print(f"bench.py: the {args.gpus}-rank launch failed (exit {proc.returncode})", file=sys.stderr)
        return proc.returncode or 1
    print(line)
    return 0


def build_inputs(fields, seed, stats_lr, stats_hr):
    """x ~ N(0,1) in standardised space, mapped back to physical
    units so the engine's fused standardise does real work.  Sample order is
    field-major, component-minor: sample 3*f + c."""
    import numpy as np
    rng = np.random.default_rng(seed)
    xs = rng.standard_normal((fields, 10, 10, 3)).astype(np.float32)
    comps = ("u", "v", "p")
    lr = np.array([stats_lr[c] for c in comps], np.float32)  # (3,2) mean,std
    hr = np.array([stats_hr[c] for c in comps], np.float32)
    raw = xs * lr[:, 1] + lr[:, 0]
    x = np.ascontiguousarray(raw.transpose(0, 3, 1, 2).reshape(fields * 3, 10, 10, 1))
    ain = np.ascontiguousarray(np.tile(lr, (fields, 1)))
    aout = np.ascontiguousarray(np.tile(hr, (fields, 1)))
    return x, ain, aout


def measured_traffic(fields, precision, out_dtype):
    """HBM bytes per launch of the dominant kernel (16-bit paths) or per step (f32 path) from the committed rocprofv3 PMC
    passes (bench.py cannot run the profiler on itself); None unless the profile was taken on this exact configuration."""
    name = "pmc_traffic_fp32.json" if precision == "fp32" else "pmc_traffic_tail.json"
    try:
        with open(os.path.join(ROOT, "profiles", name)) as f:
            t = json.load(f)
    except OSError:
        return None, None
    c = t.get("config", {})
    if (c.get("fields"), c.get("precision"), c.get("out_dtype")) != (fields, precision, out_dtype):
        return None, None
    if t.get("kernel_source_stamp") != kernel_source_stamp(name):
        return None, f"profiles/{name} is stale: its kernels' sources changed since the PMC pass (stamp {t.get('kernel_source_stamp')}); re-run tools/pmc_traffic.py"
    return t["hbm_bytes_per_launch"], t["source"]


def tail_flops(n):
    macs = 3 * 20_480_000 + 11_520_000  # ConvT#2..#4 + output conv
    return 2.0 * macs * n


def cpu_baseline(x, ain, aout, enc_w, dec_w, y_gpu, budget_s=None):
    """Reference stand-in on the host cores: the oracle's torch-CPU (oneDNN, the
    conv backend family TensorFlow uses) port of the network, Keras' default
    predict batch of 32, plus numpy pre/post as the reference does them.  The
    same leg checks the GPU outputs in `y_gpu` ({precision: first 8 samples})
    against the float64 oracle (relative L2 in standardised space)."""
    import numpy as np
    import torch
    from oracle.sr_oracle_torch import TorchSR
    if budget_s is None:   # SRCFD_BENCH_CPU_BUDGET_S: the tests shorten the sample; the line's `sample` text says what was run
        budget_s = float(os.environ.get("SRCFD_BENCH_CPU_BUDGET_S", "12"))
    model = TorchSR(enc_w, dec_w, torch.float32)
    bs = min(32, len(x))

    def std(lo, hi):
        return ((x[lo:hi] - ain[lo:hi, 0].reshape(-1, 1, 1, 1)) / ain[lo:hi, 1].reshape(-1, 1, 1, 1)).astype(np.float32)

    model.forward(std(0, bs), batch_size=bs)  # warm-up (oneDNN primitive creation)
    done, t0 = 0, time.perf_counter()
    while True:
        lo = done % (len(x) - bs + 1)
        y = model.forward(std(lo, lo + bs), batch_size=bs)
        y = y * aout[lo:lo + bs, 1].reshape(-1, 1, 1, 1) + aout[lo:lo + bs, 0].reshape(-1, 1, 1, 1)
        if np.isnan(y).any() or np.isinf(y).any():
            y = np.nan_to_num(y, nan=0.0, posinf=0.0, neginf=0.0)
        done += bs
        el = time.perf_counter() - t0
        if el >= budget_s:
            break
    # the solver-side shape of the call (configs 1 and 3): three batch-1 predicts per field, like PyCFD_ML_accelerated.py:841-876
    calls = []
    for _ in range(7):
        t1 = time.perf_counter()
        for c in range(3):
            xs1 = ((x[c:c + 1] - ain[c, 0]) / ain[c, 1]).astype(np.float32)
            _ = model.forward(xs1, batch_size=1) * aout[c, 1] + aout[c, 0]
        calls.append((time.perf_counter() - t1) * 1e3)
    # parity of the GPU paths: float64 network on the float32-standardised inputs, compared before de-standardisation
    k = 8
    ref = TorchSR(enc_w, dec_w, torch.float64).forward(std(0, k).astype(np.float64), batch_size=k).reshape(k, -1)
    rel = {}
    for prec, yg in y_gpu.items():
        ys = ((yg[:k].astype(np.float64) - aout[:k, 0].reshape(-1, 1, 1, 1)) / aout[:k, 1].reshape(-1, 1, 1, 1)).reshape(k, -1)
        rel[prec] = float(np.max(np.linalg.norm(ys - ref, axis=1) / np.linalg.norm(ref, axis=1)))
    return {
        "value": round(done / 3.0 / el, 3), "unit": "fields/s", "cores": int(torch.get_num_threads()), "kind": "port",
        "sample": f"{done} single-channel samples ({done // 3} fields) in batches of 32, f32, torch-CPU/oneDNN port of the network "
                  f"(TensorFlow/Keras not installable; SURVEY.md 8c), {el:.1f} s",
        "host_cpus": os.cpu_count(),
        "single_field_call_ms": round(float(np.median(calls)), 2),
        "gpu_rel_l2_vs_f64_oracle": rel,
    }


class Job:
    """One rank's device state."""

    def __init__(self, args):
        import numpy as np
        import torch
        import torch.distributed as dist
        self.np, self.torch, self.dist, self.args = np, torch, dist, args
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a HIP device: libsrcfd has no CPU fallback")
        self.backend = os.environ.get("SRCFD_BENCH_BACKEND", "nccl")  # nccl = RCCL; gloo only to rehearse the rank logic on fewer GPUs
        ndev = torch.cuda.device_count()
        if self.world > ndev and self.backend == "nccl":
            raise SystemExit(f"bench.py: {self.world} ranks requested but only {ndev} HIP device(s) visible")
        local_rank %= ndev
        torch.cuda.set_device(local_rank)
        self.local_rank = local_rank
        self.dev = torch.device("cuda", local_rank)
        if self.world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if self.backend == "nccl":
                dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=self.dev)
            else:
                dist.init_process_group(self.backend, rank=self.rank, world_size=self.world)
        self.world_reported = dist.get_world_size() if self.world > 1 else 1
        self.srcfd = importlib.import_module("sr-for-cfd_amd")
        self.synth = importlib.import_module("sr-for-cfd_amd.synth")
        self.shard = importlib.import_module("sr-for-cfd_amd.shard")
        self.enc_w = self.srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1).weights()   # real trained encoder (reference checkout)
        self.dec_w = self.synth.synthetic_decoder_weights(1)                              # decoder .h5 absent upstream -> random init
        self.model = self.srcfd.SRModel.from_weights(self.enc_w, self.dec_w, device=local_rank)
        self.stats_lr, self.stats_hr = self.srcfd.load_stats(STATS_TXT, 10, 400)
        self.x_h, self.ain_h, self.aout_h = build_inputs(args.fields, seed=self.rank, stats_lr=self.stats_lr, stats_hr=self.stats_hr)
        self.n = self.x_h.shape[0]
        self.x = torch.from_numpy(self.x_h).to(self.dev)
        self.ain = torch.from_numpy(self.ain_h).to(self.dev)
        self.aout = torch.from_numpy(self.aout_h).to(self.dev)
        self.bad = torch.zeros(1, dtype=torch.int64, device=self.dev)
        # One-time set-up of every leg's precision (operand packs, activation workspaces) happens here, through the ABI's
        # explicit reserve call, not lazily inside a leg's first warm-up step: a leg then starts on a GPU that the previous
        # leg has just left, instead of one that idled through host-side weight packing and hipMalloc.
        parity_legs = args.full and not args.no_extras and args.precision not in ("fp32", "fp32x3")
        for prec in dict.fromkeys((["fp32", "fp32x3"] if parity_legs else []) + [args.precision]):
            self.model.precision = prec
            self.model.reserve(self.n)
        self.y_out = {}

    def out_buffer(self, out_dtype):
        torch = self.torch
        if out_dtype not in self.y_out:
            odt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[out_dtype]
            self.y_out[out_dtype] = torch.empty((self.n, 400, 400, 1), dtype=odt, device=self.dev)
        return self.y_out[out_dtype]

    def barrier(self):
        if self.world > 1:
            self.dist.barrier()

    def timed(self, step, steps, warmup, pre_ms=0.0, pre_steps=0):
        """`warmup` untimed + exactly `steps` timed calls of `step`, bracketed by barrier + synchronize on both
        sides; returns the MAX over ranks of the seconds the timed calls took.  `pre_ms` > 0: BEFORE the counted warm-up
        steps, untimed steps are issued until that much wall time has passed -- the first ~50 ms after an idle spell run ~10 %
        slower (clock ramp), and with the driver's `--steps 20 --warmup 5` the whole 15 ms timed region would sit
        inside it.  The counted steps and warm-up stay exactly as given.  self.last_rank_ms = (min, max) over ranks of the
        per-step time, so a straggler is visible in an N > 1 line."""
        torch = self.torch
        for _ in range(pre_steps):    # steps that contain a collective are pre-warmed by COUNT: every rank must issue the same number
            step()
        if pre_ms > 0:
            t_pre = time.perf_counter()
            while (time.perf_counter() - t_pre) * 1e3 < pre_ms:
                for _ in range(4):
                    step()
                torch.cuda.synchronize()
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        self.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        mine = time.perf_counter() - t0
        self.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        dev = self.dev if self.backend == "nccl" else None
        self.last_rank_ms = (round(-self.shard.max_over_ranks(-mine, device=dev) / steps * 1e3, 4),
                             round(self.shard.max_over_ranks(mine, device=dev) / steps * 1e3, 4))
        return self.shard.max_over_ranks(dt, device=dev)

    def kernel_profile(self, step, reps):
        """Per-step kernel times from HIP events recorded by the engine on the launch stream around every
        launch: a step's launches of one name are SUMMED (the f32 path runs 768 samples as 3 chunks of 256),
        then averaged over `reps` steps."""
        np = self.np
        self.model.set_profiling(True)
        acc = {}
        for _ in range(reps):
            step()
            per_step = {}
            for name, ms in self.model.get_profile():
                per_step[name] = per_step.get(name, 0.0) + ms
            for name, ms in per_step.items():
                acc.setdefault(name, []).append(ms)
        self.model.set_profiling(False)
        return {k: round(float(np.mean(v)), 4) for k, v in acc.items()}

    # -- the SR batch (config 2) at one precision -------------------------------------------------------------
    def run_sr(self, precision, out_dtype, steps, warmup, keep=None):
        """keep: sample indices whose results of the last timed step are copied to the host (self.kept) before anything
        else runs on the result buffer."""
        torch, args = self.torch, self.args
        self.model.precision = precision
        y = self.out_buffer(out_dtype)     # one result buffer per output type, shared by the legs (allocated once)
        self.bad.zero_()

        def step():
            self.model.predict_device(self.x, y, in_affine=self.ain, out_affine=self.aout, nan_guard=True, nonfinite=self.bad)

        dt = self.timed(step, steps, warmup, pre_ms=PRE_WARM_MS)
        if keep is not None:
            self.kept = y[torch.as_tensor(keep, device=self.dev)].float().cpu().numpy()
        ms = dt / steps * 1e3
        rec = {"value": round(self.shard.aggregate_throughput(args.fields, self.world, ms * 1e-3), 2), "unit": "fields/s",
               "ms_per_step": round(ms, 4), "steps": steps, "dtype": precision, "out_dtype": out_dtype,
               "ms_per_step_rank_min_max": list(self.last_rank_ms), "untimed_pre_warm_ms": PRE_WARM_MS,
               "tflops_model": round(2.0 * MACS_PER_SAMPLE * self.n * self.world / (ms * 1e-3) / 1e12, 2),
               "nonfinite": int(self.bad.item()), "last_plan": self.model.last_plan()}   # which kernels the timed calls ran (srcfd_model_last_plan)
        if self.rank == 0 and args.full:   # the per-kernel pass is a run of its own: --full only
            kernels = self.kernel_profile(step, max(3, min(steps, 10)))
            tot = sum(kernels.values())
            rec["kernels_ms"] = kernels
            rec["kernels_ms_sum"] = round(tot, 4)
            rec["launch_gap_ms"] = round(ms - tot, 4)
            if tot > ms * 1.10:   # event records between launches add a few per cent; more means the profile is not one step
                raise SystemExit(f"bench.py: kernel times ({tot:.3f} ms) exceed the step ({ms:.3f} ms): profile is not per step")
            # The per-kernel times come from an event-instrumented pass that runs a few per cent slower than the timed step (an event
            # record between every two launches).  What the roofline divides by is the kernel's share of the TIMED step: scaled down
            # whenever the instrumented sum exceeds the step, so that the kernels of a step never add up to more than the step.
            in_step = min(1.0, ms / tot) if tot > 0 else 1.0
            rec["kernels_ms_in_step_scale"] = round(in_step, 4)
            if precision in ("bf16", "f16"):
                dom = "tail(convT2-4+out)"
                fl = tail_flops(self.n)
                dom_ms = kernels[dom] * in_step
                ach = fl / (dom_ms * 1e-3) / 1e12
                traffic, traffic_src = measured_traffic(args.fields, precision, out_dtype)
                # 2 240 000 swish activations per sample in this kernel; 9.58 ns of SIMD time per 64 of them incl. the 16-bit pack
                # (profiles/r03/a_microbench9...: the kernel's own instruction mix, 4 waves per SIMD, wall time), 1024 SIMDs
                floor = self.n * 2_240_000 / 64 * 9.58e-9 / 1024 * 1e3
                rec["roofline"] = {
                    "bound": "mfma", "kernel": dom, "achieved": round(ach, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(ach / PEAK_BF16_TFLOPS, 4), "traffic": traffic, "traffic_unit": "bytes/launch (HBM, PMC)",
                    "traffic_source": traffic_src,
                    "algorithmic_bytes_per_launch": self.n * 160000 * (2 + (4 if out_dtype == "f32" else 2)),
                    "avg_launch_ms": round(dom_ms, 4), "avg_launch_ms_event_pass": kernels[dom], "algorithmic_flops_per_launch": fl,
                    # what actually binds (not expressible as "hbm" | "mfma"): the vector unit's swish stream
                    "valu_swish_floor_ms": round(floor, 4), "frac_of_valu_swish_floor": round(floor / dom_ms, 4),
                    "note": "swish = 2 transcendentals per activation: exact swish caps this network at ~0.28 of the MFMA peak on the "
                            "vector unit (DESIGN.md 4.2); bf16 MFMAs hide under the swish stream of the wave that issues them, not under "
                            "another wave's (DESIGN.md 4.2b, profiles/r03/a_microbench9...)"}
            else:
                # whole f32 step: all 768 samples' FLOPs over the SUM of every launch of the step (all chunks)
                fl = 2.0 * MACS_PER_SAMPLE * self.n
                ach = fl / (tot * in_step * 1e-3) / 1e12
                traffic, traffic_src = measured_traffic(args.fields, precision, out_dtype)
                rec["roofline"] = {"bound": "mfma", "kernel": "all f32 kernels of one step (sum over all launches)", "achieved": round(ach, 2),
                                   "peak": PEAK_FP32_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_FP32_TFLOPS, 4), "traffic": traffic,
                                   "traffic_unit": "bytes/step (HBM, PMC)", "traffic_source": traffic_src,
                                   "algorithmic_bytes_per_launch": self.n * (100 + 160000) * 4,
                                   "avg_launch_ms": round(tot * in_step, 4), "avg_launch_ms_event_pass": round(tot, 4), "algorithmic_flops_per_launch": fl,
                                   "note": "f32-input MFMAs and vector instructions of a SIMD do not overlap on gfx950, neither across waves nor in one "
                                           "wave's stream (profiles/r02/d_microbench8...): the swish / output-conv vector work of this path is paid on "
                                           "top of the MFMA time (the 16-bit MFMAs differ: DESIGN.md 4.2b)"}
        return rec, y

    # -- config 4: training step ---------------------------------------------------------------------------------
    def run_train(self, steps=30, warmup=3, batch=8):
        """BASELINE config 4: the weak-scaling leg (micro-batch 8 per GPU = the reference's BATCH_SIZE,
        sr-ae-conv.ipynb:c386-388, global batch 8 G) is the record's `value`; `strong` holds the global-batch-256 regime
        (256 / G samples per rank and step): accumulated from micro-batches of 8, and from calls of up to 32 samples."""
        np, torch = self.np, self.torch
        tr = importlib.import_module("sr-for-cfd_amd.train")
        ds = importlib.import_module("sr-for-cfd_amd.datasets")
        enc, dec = self.synth.keras_default_init(0)                     # identical replicas: same seed on every rank
        model = self.srcfd.SRModel.from_weights(enc, dec, device=self.local_rank)
        # set-up (allocations) first, agreed on by every rank BEFORE anything enters a collective: a rank that cannot allocate must
        # not leave the others waiting in an all-reduce
        ok = 1
        t = t32 = None
        try:
            t = tr.Trainer(model, max_batch=batch)
            t32 = tr.Trainer(model, max_batch=32)
            # the notebook's own dummy recipe (sr-ae-conv.ipynb:c72-91): x_hr ~ N(0,1), x_lr = avg_pool(x_hr, 40)
            rng = np.random.default_rng(1000 + self.rank)
            y_h = rng.standard_normal((32, 400, 400, 1)).astype(np.float32)
            x32 = torch.from_numpy(ds.avg_pool(y_h, 40)).to(self.dev)
            y32 = torch.from_numpy(y_h).to(self.dev)
        except Exception as e:   # noqa: BLE001
            ok, err = 0, f"{type(e).__name__}: {e}"[:200]
        if self.world > 1:
            flag = torch.tensor([ok], dtype=torch.int32, device=self.dev if self.backend == "nccl" else "cpu")
            self.dist.all_reduce(flag, op=self.dist.ReduceOp.MIN)
            all_ok = int(flag.item())
        else:
            all_ok = ok
        if not all_ok:
            for h_ in (t, t32):
                if h_ is not None:
                    h_.close()
            model.close()
            raise RuntimeError("training set-up failed on " + ("this rank: " + err if not ok else "another rank"))
        x, y = x32[:batch].contiguous(), y32[:batch].contiguous()
        gb = batch * self.world

        def step():
            # the product's own optimisation step (train.py Trainer.step): forward + backward storing the gradients (no zero-fill
            # launches), the flat all-reduce -- the step's only collective, RCCL when backend == nccl -- and Adam; no loss read-back
            t.step(x, y, gb, return_loss=False)

        # like the SR legs, untimed steps first (the leg starts on a device that idled through the trainers' set-up; its 15 ms timed
        # region would otherwise sit inside the clock ramp -- 0.549 vs 0.505 ms per step measured); by count, not by wall time: the
        # step holds a collective.  Round 3's line had none
        dt = self.timed(step, steps, warmup, pre_steps=100)
        ms = dt / steps * 1e3
        t.sse.zero_()
        t.forward_backward(x, y, gb)
        loss = float(t.sse.item()) / (batch * 160000)
        flops_per_sample = 3 * 2 * MACS_PER_SAMPLE
        rec = {"metric": "conv-AE training samples/s (10x10->400x400, f32, Adam; BASELINE config 4)", "value": round(gb / (ms * 1e-3), 2),
               "unit": "samples/s", "ms_per_step": round(ms, 4), "steps": steps, "warmup": warmup, "micro_batch": batch, "global_batch": gb,
               "scaling": "weak", "dtype": "f32", "params": t.n_params, "collective": "none" if self.world == 1 else
               f"all_reduce(sum) of {t.n_params} f32 per step, backend {self.backend}",
               "tflops_model": round(flops_per_sample * gb / (ms * 1e-3) / 1e12, 2),
               "frac_f32_mfma_peak": round(flops_per_sample * batch / (ms * 1e-3) / 1e12 / PEAK_FP32_TFLOPS, 4),
               "ms_per_step_rank_min_max": list(self.last_rank_ms), "untimed_pre_warm_steps": 100,
               "loss_finite": bool(np.isfinite(loss))}

        # strong scaling: global batch 256, 256 / G samples per rank and optimiser step (sr-ae-conv.ipynb:c386-388 BATCH_SIZE scaled
        # to the node).  Two ways to run a rank's share: micro-batches of 8 accumulated (the weak leg's kernels), and
        # calls of up to 32 samples (the regime where the training kernels stop being launch latency)
        GB = 256
        per_rank = GB // self.world if GB % self.world == 0 else 0
        strong = {"global_batch": GB, "samples_per_rank": per_rank}
        if per_rank >= 8 and per_rank % 8 == 0:
            for name, trn, mb in (("micro8", t, 8), ("calls_of_up_to_32", t32, min(32, per_rank))):
                calls = per_rank // mb

                def sstep(trn=trn, mb=mb, calls=calls):
                    for c in range(calls):     # the first call of a step stores the gradients and re-packs the (new) parameters, the others add
                        lo = (c * mb) % 32
                        trn.forward_backward(x32[lo:lo + mb], y32[lo:lo + mb], GB, overwrite=(c == 0), same_params=(c > 0))
                    tr.allreduce_sum_(trn.grads)
                    trn.apply_adam()

                sdt = self.timed(sstep, max(4, steps // 5), 2, pre_steps=3)
                sms = sdt / max(4, steps // 5) * 1e3
                strong[name] = {"ms_per_step": round(sms, 4), "samples_per_s": round(GB / (sms * 1e-3), 1), "calls_per_step": calls, "call_batch": mb,
                                "frac_f32_mfma_peak": round(flops_per_sample * per_rank / (sms * 1e-3) / 1e12 / PEAK_FP32_TFLOPS, 4),
                                "ms_per_step_rank_min_max": list(self.last_rank_ms)}
        else:
            strong["skipped"] = f"256 is not a multiple of 8 x {self.world} ranks"
        rec["strong"] = strong
        t.close()
        t32.close()
        model.close()
        return rec

    # -- config 5: tiled SR -------------------------------------------------------------------------------------
    def run_tiled(self, steps=20, warmup=3, keep=False):
        """One 40x40x3 field = 4x4 tiles x 3 components = 48 samples -> 1600x1600x3, f16 operands; the tile samples are
        sharded contiguously over the ranks (shard.shard_range), no collective in the timed region."""
        np, torch = self.np, self.torch
        rng = np.random.default_rng(5)
        field = rng.standard_normal((40, 40, 3)).astype(np.float32)
        tiles = np.ascontiguousarray(field.reshape(4, 10, 4, 10, 3).transpose(0, 2, 4, 1, 3).reshape(48, 10, 10, 1))
        lo, hi = self.shard.shard_range(48, self.rank, self.world)
        n = hi - lo
        self.model.precision = "f16"
        x = torch.from_numpy(tiles[lo:hi]).to(self.dev)
        y = torch.empty((max(n, 1), 400, 400, 1), dtype=torch.float32, device=self.dev)

        def step():
            if n:
                self.model.predict_device(x, y[:n], nan_guard=True, nonfinite=self.bad)

        dt = self.timed(step, steps, warmup, pre_ms=PRE_WARM_MS / 2)
        if keep:
            self.kept = y[:n].cpu().numpy()
        ms = dt / steps * 1e3
        return {"ms_per_step_rank_min_max": list(self.last_rank_ms), "metric": "tiled SR fields/s (40x40x3 -> 1600x1600x3 via 4x4 tiles; BASELINE config 5)", "value": round(1.0 / (ms * 1e-3), 2),
                "unit": "fields/s", "ms_per_field": round(ms, 4), "steps": steps, "warmup": warmup, "dtype": "f16", "tile_samples": 48,
                "tile_samples_this_rank": n, "scaling": "strong", "mpix_per_s": round(1600 * 1600 * 3 / (ms * 1e-3) / 1e6, 1)}

    # -- host-buffer entry ---------------------------------------------------------------------------------------
    def run_host_io(self):
        """srcfd_predict (numpy in -> numpy out): what a solver gets when it hands over host arrays.  `value` of the
        headline never includes any of this."""
        np = self.np
        out = {}
        self.model.precision = "bf16"
        for n in (3, self.n):
            x = self.x_h[:n]
            ai, ao = self.ain_h[:n], self.aout_h[:n]
            eng = importlib.import_module("sr-for-cfd_amd.engine")
            eng._result_pool.trim()                      # the first call below pays the page-locked allocation (hipHostMalloc)
            t0 = time.perf_counter()
            y = self.model.predict(x, in_affine=ai, out_affine=ao, nan_guard=True)
            first = time.perf_counter() - t0
            del y
            fresh = []
            for _ in range(3):
                t0 = time.perf_counter()
                y = self.model.predict(x, in_affine=ai, out_affine=ao, nan_guard=True)
                fresh.append(time.perf_counter() - t0)
            yp = np.empty(y.shape, np.float32)
            yp.fill(0)                      # a caller-owned pageable array, pages already touched
            reused = []
            for _ in range(3):
                t0 = time.perf_counter()
                self.model.predict(x, in_affine=ai, out_affine=ao, nan_guard=True, out=yp)
                reused.append(time.perf_counter() - t0)
            out[f"samples_{n}"] = {"first_call_allocating_ms": round(first * 1e3, 3), "new_array_from_pool_ms": round(min(fresh) * 1e3, 3),
                                   "reused_result_ms": round(min(reused) * 1e3, 3),
                                   "fields_per_s_fresh": round(n / 3 / min(fresh), 1), "fields_per_s_reused": round(n / 3 / min(reused), 1),
                                   "d2h_GBps_fresh": round(y.nbytes / min(fresh) / 1e9, 2), "d2h_GBps_reused": round(y.nbytes / min(reused) / 1e9, 2)}
            del y, yp
        out["note"] = ("first_call_allocating: the pool is empty, the call pays hipHostMalloc; new_array_from_pool (`fresh`): predict() returns a new "
                       "array over a RECYCLED page-locked buffer (copy of chunk i overlaps the kernels of chunk i+1), min of 3; reused: out= a "
                       "caller-owned pageable array (staged copy, nothing overlaps)")
        return out


def dry_run(args, env):
    """SRCFD_BENCH_DRYRUN=1: the rank plumbing only (process group, barrier, MAX over ranks, the legs' shard arithmetic, the
    all-or-none agreement after a leg, rank 0's line) with no device work, so that `--gpus N` -- N = 8 included -- can be rehearsed
    on a box without GPUs (tests/test_distributed.py).  `value` is null."""
    import torch
    import torch.distributed as dist
    shard = importlib.import_module("sr-for-cfd_amd.shard")
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dist.barrier()
    t = shard.max_over_ranks(float(rank + 1))
    tmin = -shard.max_over_ranks(-float(rank + 1))
    lo, hi = shard.shard_range(48, rank, world)
    counts = torch.zeros(world, dtype=torch.int64)
    counts[rank] = hi - lo
    # what every rank would hold: the headline batch, the f32 parity workspace, the trainers -- host-side estimate of the
    # device bytes reserve() asks for per rank (8 ranks share one host's memory for their staging copies only)
    fail = torch.tensor([1 if os.environ.get("SRCFD_BENCH_DRYRUN_FAIL_RANK", "") == str(rank) else 0], dtype=torch.int32)
    if world > 1:
        dist.all_reduce(counts)
        dist.all_reduce(fail, op=dist.ReduceOp.MAX)
    per_rank_256 = 256 // world if 256 % world == 0 else 0
    budget = None
    if rank == 0:
        # What the N ranks of one host would hold: every rank reserves the workspaces of every precision its legs use and keeps its
        # input / result buffers; rank 0 alone runs the host_io and CPU legs.  Sizes come from the library (srcfd_model_footprint on a
        # host-only handle: nothing is allocated) and are set against the host's memory and one MI355X's 288 GB.
        try:
            srcfd = importlib.import_module("sr-for-cfd_amd")
            synth = importlib.import_module("sr-for-cfd_amd.synth")
            enc_w = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1).weights()
            mdl = srcfd.SRModel.from_weights(enc_w, synth.synthetic_decoder_weights(1), device=-1)
            n = 3 * args.fields
            tile_n = int(counts.max().item()) if world > 1 else 48
            legs = {"headline_bf16": mdl.footprint(n, "bf16"), "parity_fp32": mdl.footprint(n, "fp32"), "tiled_f16": mdl.footprint(tile_n, "f16")}
            dev = sum(v["device_workspace"] for v in legs.values()) + 3 * legs["parity_fp32"]["device_weights"]
            dev += n * (100 * 4 + 16) + n * 160000 * 4     # the rank's resident inputs + one f32 result buffer shared by the legs
            dev += legs["headline_bf16"]["device_host_entry_staging"]          # host_io (rank 0): staging of the host-buffer entry
            host_rank0 = 2 * legs["headline_bf16"]["host_result"]               # host_io: one result from the page-locked pool + one pageable array
            host_every = n * (100 * 4 + 16)                                      # inputs kept on the host
            runtime_per_process = 4 << 30                                         # torch + HIP runtime + code objects, measured ~3 GB resident
            mem_total = None
            for ln in open("/proc/meminfo"):
                if ln.startswith("MemTotal:"):
                    mem_total = int(ln.split()[1]) * 1024
            host_all = world * (host_every + runtime_per_process) + host_rank0
            budget = {"per_rank_device_bytes": int(dev), "device_capacity_bytes": 288 * 10**9, "host_bytes_all_ranks": int(host_all),
                      "host_pinned_bytes_rank0": int(legs["headline_bf16"]["host_result"]), "host_mem_total_bytes": mem_total,
                      "fits": bool(dev < 288 * 10**9 and (mem_total is None or host_all < mem_total)), "legs": legs,
                      "not_counted": "the trainers of the train leg (f32 activations of a micro-batch of 8-32 samples: < 2 GB per rank)"}
        except Exception as e:   # noqa: BLE001 -- the rehearsal must not die on an estimate
            budget = {"error": f"{type(e).__name__}: {e}"}
    # the tail of a real --full run: rank 0's own legs (host entry, CPU stand-in, oracle check) while the others wait at one barrier
    cpu = None
    if rank == 0 and args.full:
        try:
            import numpy as np
            stats_lr, stats_hr = srcfd.load_stats(STATS_TXT, 10, 400)
            x_h, ain_h, aout_h = build_inputs(11, seed=0, stats_lr=stats_lr, stats_hr=stats_hr)    # 33 samples: one batch of 32
            cpu = cpu_baseline(x_h, ain_h, aout_h, enc_w, synth.synthetic_decoder_weights(1), {}, budget_s=0.2)
        except Exception as e:   # noqa: BLE001
            cpu = {"error": f"{type(e).__name__}: {e}"}
    if world > 1:
        dist.barrier()
    if rank == 0:
        print(json.dumps({"metric": "SR fields/sec (10x10->400x400, 3-ch) @batch256", "value": None, "unit": "fields/s", "dry_run": True,
                          "cpu_baseline": cpu,
                          "n_gpus": world, "world_size_reported": dist.get_world_size() if world > 1 else 1, "steps": args.steps,
                          "warmup": args.warmup, "max_over_ranks": t, "min_over_ranks": tmin, "tile_samples_covered": int(counts.sum().item()),
                          "tile_samples_per_rank": [int(c) for c in counts], "fields_total": args.fields * world,
                          "train": {"global_batch": 8 * world, "strong": {"global_batch": 256, "samples_per_rank": per_rank_256}},
                          "leg_failed_somewhere": bool(fail.item()), "budget": budget, "env": env}))
    if world > 1:
        dist.destroy_process_group()


def main():
    argv = sys.argv[1:]
    args = parse_args(argv)
    env = srcfd_env()
    bad_env = non_default_switches(env)
    if bad_env and os.environ.get("SRCFD_BENCH_ALLOW_DIAG", "0") in ("", "0"):
        raise SystemExit(f"bench.py: {bad_env} set: diagnostic switches skip work or add synchronisation, A/B switches select another "
                         "implementation than the shipped one; refusing to report a number (SRCFD_BENCH_ALLOW_DIAG=1 reports an INVALID line)")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args, argv))
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world_env}; launch one rank per GPU (or let --gpus start them)")

    if os.environ.get("SRCFD_BENCH_DRYRUN", "0") not in ("", "0"):
        return dry_run(args, env)

    job = Job(args)
    torch, np = job.torch, job.np
    extras = args.full and not args.no_extras
    cpu_leg = args.full and not args.no_cpu_baseline
    dump = args.dump_outputs is not None and job.rank == 0

    if args.workload == "tiled":
        rec = job.run_tiled(args.steps, args.warmup, keep=dump)
        if dump:
            write_outputs(args.dump_outputs, {"y": job.kept, "y_sample_index": np.arange(len(job.kept), dtype=np.float64)})
        if job.rank == 0:
            print(json.dumps({"metric": rec["metric"], "value": rec["value"], "unit": rec["unit"], "n_gpus": job.world,
                              "world_size_reported": job.world_reported, "steps": args.steps, "warmup": args.warmup,
                              "ms_per_step": rec["ms_per_field"], "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
                              "dtype": "f16", "data": "synthetic",
                              "config": {"workload": "BASELINE config 5: 40x40x3 -> 1600x1600x3 via 4x4 non-overlapping 10x10 tiles "
                                                     "(48 single-channel samples), same weights, tile samples sharded over the ranks",
                                         "parallelism": f"tile-sharded x{job.world}, no collective"},
                              "detail": rec, "env": env}))
        if job.world > 1:
            job.dist.destroy_process_group()
        return

    y_gpu = {}
    parity = parity_x3 = train = tiled = host_io = None
    extra_errors = {}

    def leg(name, fn):
        """A sub-record must never cost the headline: an exception in one is recorded in the line instead of ending the run.  With
        several ranks the legs' collectives must be entered by all or none: a leg does its allocations first and agrees on them
        (run_train); after every leg the ranks agree on its outcome, so a failure anywhere is recorded everywhere."""
        res, failed = None, 0
        try:
            res = fn()
        except Exception as e:   # noqa: BLE001
            extra_errors[name] = f"{type(e).__name__}: {e}"[:300]
            failed = 1
        if job.world > 1:
            flag = torch.tensor([failed], dtype=torch.int32, device=job.dev if job.backend == "nccl" else "cpu")
            job.dist.all_reduce(flag, op=job.dist.ReduceOp.MAX)
            if int(flag.item()) and not failed:
                extra_errors[name] = "failed on another rank"
                res = None
        return res

    # Order of the legs: the f32 parity path first (parity is the gate; it also means the headline's W warm-up steps do not
    # start on a GPU that has idled through model loading and weight packing), then the headline, then the other sub-records.
    if extras and args.precision != "fp32":
        def _parity():
            rec, y_par = job.run_sr("fp32", "f32", max(5, min(args.steps, 20)), min(args.warmup, 3))
            if job.rank == 0 and cpu_leg:
                y_gpu["fp32"] = y_par[:8].cpu().numpy()
            return rec
        parity = leg("parity_path", _parity)

        def _parity_x3():   # the same batch at SRCFD_PREC_FP32X3: f32-grade, ConvT#0 / ConvT#1 as six bf16 MFMAs on exactly split operands
            rec, y_par = job.run_sr("fp32x3", "f32", max(5, min(args.steps, 20)), min(args.warmup, 3))
            if job.rank == 0 and cpu_leg:
                y_gpu["fp32x3"] = y_par[:8].cpu().numpy()
            if "roofline" in rec:   # rank 0 only
                rec["roofline"]["note"] = ("algorithmic f32 FLOPs over the f32 MFMA peak, as for parity_path -- but ConvT#0 / ConvT#1 (45 % of the MACs) run as 6 bf16 "
                    "MFMAs per f32 product (kernels_x3.hip), the rest on the f32 kernels: a mixed-pipe number, for comparison with parity_path only")
            return rec
        parity_x3 = leg("parity_path_x3", _parity_x3)

    pci = None
    if args.full:
        try:
            pr = torch.cuda.get_device_properties(job.local_rank)
            pci = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
        except Exception:   # noqa: BLE001
            pass
    gpu_before = gpu_state(pci) if job.rank == 0 and args.full else None
    keep = dump_index(job.n) if dump else None
    head, y_head = job.run_sr(args.precision, args.out_dtype, args.steps, args.warmup, keep=keep)
    gpu_after = gpu_state(pci) if job.rank == 0 and args.full else None
    if dump:
        write_outputs(args.dump_outputs, {"y": job.kept, "y_sample_index": keep.astype(np.float64)})
        del job.kept
    if job.rank == 0 and cpu_leg and args.out_dtype == "f32":
        y_gpu[args.precision] = y_head[:8].cpu().numpy()
    del y_head

    if extras:
        torch.cuda.empty_cache()
        train = leg("train", job.run_train)
        tiled = leg("tiled", job.run_tiled)
    # Rank 0's own legs come after every collective leg, for any N (an N > 1 line without cpu_baseline or the oracle
    # check reads as unmeasured): the host-buffer entry, the CPU stand-in and the float64-oracle check of both paths' first samples.
    # The other ranks wait at ONE barrier behind them (gloo / RCCL barriers have minutes of patience; these legs take ~20 s).
    cpu = None
    if job.rank == 0:
        if extras:
            try:
                host_io = job.run_host_io()
            except Exception as e:   # noqa: BLE001
                extra_errors["host_io"] = f"{type(e).__name__}: {e}"[:300]
        if cpu_leg:
            try:
                cpu = cpu_baseline(job.x_h, job.ain_h, job.aout_h, job.enc_w, job.dec_w, y_gpu)
                for rec_, key_ in ((parity, "fp32"), (parity_x3, "fp32x3")):
                    if rec_ is not None and key_ in cpu["gpu_rel_l2_vs_f64_oracle"]:
                        rec_["rel_l2_vs_f64_oracle"] = cpu["gpu_rel_l2_vs_f64_oracle"][key_]
                        rec_["tolerance"] = 1e-5
            except Exception as e:   # noqa: BLE001
                extra_errors["cpu_baseline"] = f"{type(e).__name__}: {e}"[:300]
    job.barrier()

    # the fastest measured path whose first samples sit within north_star's 1e-5 of the float64 oracle (checked in THIS run)
    best_1e5 = None
    if job.rank == 0:
        for rec_, key_ in ((parity, "fp32"), (parity_x3, "fp32x3")):
            if rec_ is not None and rec_.get("rel_l2_vs_f64_oracle") is not None and rec_["rel_l2_vs_f64_oracle"] <= 1e-5 and \
                    (best_1e5 is None or rec_["value"] > best_1e5["value"]):
                best_1e5 = {"precision": key_, "value": rec_["value"], "unit": "fields/s", "ms_per_step": rec_["ms_per_step"],
                            "rel_l2_vs_f64_oracle": rec_["rel_l2_vs_f64_oracle"], "tolerance": 1e-5,
                            "record": "parity_path" if key_ == "fp32" else "parity_path_x3"}

    if job.rank == 0:
        out = {
            "metric": "SR fields/sec (10x10->400x400, 3-ch) @batch256", "value": head["value"], "unit": "fields/s",
            "n_gpus": job.world, "world_size_reported": job.world_reported, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.precision, "data": "synthetic",
            "config": {"workload": "BASELINE config 2: batched SR inference, 256 fields x (10,10,3)->(400,400,3) per GPU = 768 "
                                   "single-channel encoder_10+decoder_400 passes, fused standardise/de-standardise/NaN guard",
                       "fields_per_gpu": args.fields, "samples_per_gpu": job.n, "out_dtype": args.out_dtype,
                       "weights": "encoder: reference multiBC .h5; decoder: random init seed 1 (reference decoder .h5 absent)",
                       "parallelism": f"sample-sharded x{job.world}, no collective", "backend": job.backend if job.world > 1 else None},
            "tflops_model": head["tflops_model"], "nonfinite": head["nonfinite"], "last_plan": head.get("last_plan"),
            "ms_per_step_rank_min_max": head.get("ms_per_step_rank_min_max"), "untimed_pre_warm_ms": head.get("untimed_pre_warm_ms"),
            "full": args.full, "env": env,
        }
        if args.full:
            out.update({
                "kernels_ms": head.get("kernels_ms"), "kernels_ms_sum": head.get("kernels_ms_sum"), "kernels_ms_in_step_scale": head.get("kernels_ms_in_step_scale"),
                "launch_gap_ms": head.get("launch_gap_ms"),
                "roofline": head.get("roofline"),
                "cpu_baseline": cpu,
                "parity_path": parity, "parity_path_x3": parity_x3, "fastest_path_within_1e-5": best_1e5, "train": train, "tiled": tiled, "host_io": host_io,
                "env": dict(env, gpu_state_before_headline=gpu_before, gpu_state_after_headline=gpu_after),
            })
        if extra_errors:
            out["sub_record_errors"] = extra_errors
        if bad_env:
            out["INVALID_diagnostic_run"] = bad_env   # SRCFD_BENCH_ALLOW_DIAG=1: tools/ablate*.sh and A/B timing only
        print(json.dumps(out))
    if job.world > 1:
        job.dist.destroy_process_group()


if __name__ == "__main__":
    main()
