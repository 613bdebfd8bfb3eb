"""Times the device fine-mesh solver (srcfd_fine_solver_*) on the reference's two 400x400 configurations and prints one JSON line:
LDC (QUICK, Re 1000, double lid; PyCFD_ML_accelerated.py __main__) and BFS (UPWIND, Re 400, lx 10, ly 3; bfs_ml_accelerated.py
__main__).  Per configuration: ms per outer iteration, sweeps per inner solve, operations enqueued against sweeps executed,
us per sweep launch against the 1.45 us dependent-launch floor, and srcfd_coarse_solve (host, serial) on the same problem for
2 outer iterations as the host comparison.

    python tools/fine_solver_bench.py [--iters N] [--warmup W] [--n 400]

With --batch 1,2,4,8,16 it times the batched solver (srcfd_fine_batch_*) instead: per batch size B, B cavities (QUICK, double
lid, Re spread evenly over 100..800, from zero) as one batch, and in the same process the same cases one after the other, each in
a single-case handle of its own (a batch of one: B cases in one handle against B handles); --repeats times each, on fresh handles.  One JSON line: per B and repeat the ms per outer
iteration of the batch and of the B sequential solves, and from the batch's counters the us per sweep launch and host_syncs.

    python tools/fine_solver_bench.py --batch 1,2,4,8,16 --iters 10 --warmup 2 [--repeats 3]

With --handoff 1,8,16 it times the SR hand-off into the device state at n x n instead (real encoder, synthetic decoder; LDC, and
BFS through the back-resampler): per batch size B the wall time of one FineSolverBatch.init_from_prediction call that warm-starts
all B cases (network, [resampler,] hand-off kernel, priming, the host synchronisation at its end), and of B single-case
FineSolver.init_from_prediction calls one after the other on B handles; --repeats times each after --warmup untimed calls, handles
created outside the timed region.  --single-only times only the single-case calls, which is all a tree without the batched entry
has: run it there for the comparison.  One JSON line with every repeat in us.  On a shared machine give every invocation a time
limit of its own and chain them, e.g.

    timeout -k 10 120 python tools/fine_solver_bench.py --handoff 1,8,16 --repeats 7 > handoff.json &&
    timeout -k 10 120 python tools/fine_solver_bench.py --handoff 1,8,16 --repeats 7 --single-only > handoff_single.json

With --resident it times the resident mode (srcfd_fine_batch_set_mode, one workgroup per case) against the launch-per-sweep mode
on small meshes instead: per configuration (LDC QUICK double lid with Re spread over 100..800, BFS UPWIND Re 400), mesh of
--mesh and batch size of --batch, --repeats times each mode on a fresh handle, the two modes alternating, --warmup untimed
iterations and then --iters timed ones.  One JSON line: every repeat's ms per outer iteration of the batch, the medians and
ranges, and whether the resident median lies below the whole range of the launch mode.  --pinned adds the wall seconds of the
59 765-iteration 10x10 Re 800 run of tests/test_gpu_fine_solver.py in both modes.

    python tools/fine_solver_bench.py --resident --mesh 10,20,30,40,50,64 --batch 1,8 --iters 10 --warmup 2 [--pinned]

With --pressure sweeps|direct it times one inner pressure solver (FineSolverBatch.set_pressure_solver) on both configurations at
n x n instead: per configuration and batch size of --batch (default 1,8,16; B copies of the configuration as one batch, from zero),
--repeats times on a fresh handle, --warmup untimed iterations and then --iters timed ones.  One JSON line: every repeat's ms per
outer iteration of the batch, the median and range, and per repeat the operations enqueued and the host synchronisations of the
timed iterations.  One arm per invocation, so that arms of different libraries (SRCFD_LIB, or another checkout) can alternate;
`--pressure sweeps` passes no keyword to the solver, so the same file also runs in a tree that has no direct mode.

    python tools/fine_solver_bench.py --pressure direct --batch 1,8,16 --iters 10 --warmup 2 [--repeats 3]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(solver, warmup, iters):
    solver.run(warmup)
    c0 = solver.counters()
    t0 = time.perf_counter()
    solver.run(iters)
    dt_s = time.perf_counter() - t0
    c1 = solver.counters()
    return dt_s, {k: c1[k] - c0[k] for k in ("momentum_sweeps", "pressure_sweeps", "launches", "host_syncs")}


def batch_bench(a, fine, coarse):
    n = a.n
    out = {"mesh": f"{n}x{n}", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "floor_us_per_launch": 1.45, "batch": {}}
    for B in [int(b) for b in a.batch.split(",")]:
        res = [float(r) for r in np.linspace(100.0, 800.0, B)]
        pbs = [fine.problem(Re, n, n, 1.0, 1.0, 0.001, "QUICK", None, coarse.LDC_DOUBLE_LID) for Re in res]
        rows = []
        for _ in range(a.repeats):
            b = fine.FineSolverBatch(pbs)
            dt_s, c = _timed(b, a.warmup, a.iters)
            b.close()
            seq_s, seq_launches = 0.0, 0
            for pb in pbs:
                s = fine.FineSolver(pb)
                one_s, c1 = _timed(s, a.warmup, a.iters)
                s.close()
                seq_s += one_s
                seq_launches += c1["momentum_sweeps"] + 2 * c1["pressure_sweeps"]
            sweep_launches = c["momentum_sweeps"] + 2 * c["pressure_sweeps"]
            rows.append({
                "batch_ms_per_outer_iteration": round(1e3 * dt_s / a.iters, 3),
                "batch_ms_per_outer_iteration_per_case": round(1e3 * dt_s / a.iters / B, 3),
                "sequential_ms_per_outer_iteration": round(1e3 * seq_s / a.iters, 3),
                "batch_over_sequential": round(dt_s / seq_s, 4),
                "sweep_launches_executed": sweep_launches,
                "sequential_sweep_launches_executed": seq_launches,
                "us_per_sweep_launch": round(1e6 * dt_s / max(1, sweep_launches), 3),
                "sequential_us_per_sweep_launch": round(1e6 * seq_s / max(1, seq_launches), 3),
                "launches_issued": c["launches"],
                "host_syncs": c["host_syncs"],
            })
        out["batch"][str(B)] = {"reynolds": res, "repeats": rows}
    print(json.dumps(out))


def pressure_bench(a, fine, coarse):
    n = a.n
    bfs = {"step_height": 1.0, "h": 2.0, "Ub": 1.0}
    configs = {
        "ldc_quick_re1000_double_lid": lambda: fine.problem(1000.0, n, n, 1.0, 1.0, 0.001, "QUICK", None, coarse.LDC_DOUBLE_LID),
        "bfs_upwind_re400": lambda: fine.problem(400.0, n, n, 10.0, 3.0, 0.002, "UPWIND", None, None, bfs=bfs),
    }
    mode = {} if a.pressure == "sweeps" else {"pressure": a.pressure}
    out = {"mesh": f"{n}x{n}", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "pressure": a.pressure,
           "unit": "ms per outer iteration of the batch", "configs": {}}
    for name, make in configs.items():
        out["configs"][name] = {}
        for B in [int(b) for b in (a.batch or "1,8,16").split(",")]:
            ms, launches, syncs, sweeps = [], [], [], []
            for _ in range(a.repeats):
                b = fine.FineSolverBatch([make() for _ in range(B)], **mode)
                dt_s, c = _timed(b, a.warmup, a.iters)
                b.close()
                ms.append(round(1e3 * dt_s / a.iters, 4))
                launches.append(c["launches"])
                syncs.append(c["host_syncs"])
                sweeps.append(c["pressure_sweeps"])
            out["configs"][name][str(B)] = {"ms": ms, "median": float(np.median(ms)), "range": [min(ms), max(ms)],
                                            "launches_issued": launches, "host_syncs": syncs, "pressure_sweeps": sweeps}
    print(json.dumps(out))


def resident_bench(a, fine, coarse):
    bfs = {"step_height": 1.0, "h": 2.0, "Ub": 1.0}
    configs = {
        "ldc_quick_double_lid": lambda n, B: [fine.problem(float(Re), n, n, 1.0, 1.0, 0.001, "QUICK", None, coarse.LDC_DOUBLE_LID)
                                              for Re in np.linspace(100.0, 800.0, B)],
        "bfs_upwind_re400": lambda n, B: [fine.problem(400.0, n, n, 10.0, 3.0, 0.002, "UPWIND", None, None, bfs=bfs) for _ in range(B)],
    }
    out = {"iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "unit": "ms per outer iteration of the batch", "resident": {}}
    for name, make in configs.items():
        out["resident"][name] = {}
        for n in [int(m) for m in a.mesh.split(",")]:
            if not fine.resident_supported(n, n):
                out["resident"][name][f"{n}x{n}"] = {"supported": False}
                continue
            for B in [int(b) for b in (a.batch or "1").split(",")]:
                pbs = make(n, B)
                ms = {False: [], True: []}
                sweeps = {}
                for _ in range(a.repeats):
                    for resident in (False, True):
                        b = fine.FineSolverBatch(pbs, resident=resident)
                        dt_s, c = _timed(b, a.warmup, a.iters)
                        b.close()
                        ms[resident].append(round(1e3 * dt_s / a.iters, 4))
                        sweeps[resident] = c
                row = {"launches_ms": ms[False], "resident_ms": ms[True],
                       "launches_median": float(np.median(ms[False])), "launches_range": [min(ms[False]), max(ms[False])],
                       "resident_median": float(np.median(ms[True])), "resident_range": [min(ms[True]), max(ms[True])],
                       "resident_median_below_launches_range": bool(np.median(ms[True]) < min(ms[False])),
                       "launches_over_resident": round(float(np.median(ms[False]) / np.median(ms[True])), 2),
                       "pressure_sweeps": sweeps[True]["pressure_sweeps"], "momentum_sweeps": sweeps[True]["momentum_sweeps"],
                       "resident_launches": sweeps[True]["launches"], "launch_mode_launches": sweeps[False]["launches"]}
                out["resident"][name].setdefault(f"{n}x{n}", {})[str(B)] = row
    if a.pinned:
        out["pinned_10x10_re800_59765_iterations_s"] = {}
        for resident in (False, True):
            s = fine.FineSolver(fine.problem(800.0, 10, 10, bc=coarse.LDC_DOUBLE_LID, convergence_criteria={"u": 0.0, "v": 0.0, "p": 0.0}),
                                resident=resident)
            t0 = time.perf_counter()
            s.run(59765)
            out["pinned_10x10_re800_59765_iterations_s"]["resident" if resident else "launches"] = round(time.perf_counter() - t0, 3)
            s.close()
    print(json.dumps(out))


def handoff_bench(a, fine, coarse):
    srcfd = importlib.import_module("sr-for-cfd_amd")
    synth = importlib.import_module("sr-for-cfd_amd.synth")
    rs = importlib.import_module("sr-for-cfd_amd.resample")
    n = a.n
    stem = "swish_trained_upto_700_multiBC"
    enc_w = srcfd.SRModel.load_h5(os.path.join(a.golden, f"vanilla_encoder10_to_400_{stem}.h5"), None, device=-1).weights()
    model = srcfd.SRModel.from_weights(enc_w, synth.synthetic_decoder_weights(1), device=0)
    lr, hr = srcfd.load_stats(os.path.join(a.golden, f"standardization_stats_10to400_{stem}.txt"), 10, 400)
    ain1, aout1 = (np.array([st[c] for c in "uvp"], np.float32) for st in (lr, hr))
    if model.output_shape[:2] != (n, n):
        raise SystemExit(f"--handoff needs --n {model.output_shape[0]}: the mesh of the decoder's output")

    def inputs(name):
        cf = srcfd.read_coarse_fields(os.path.join(a.golden, name))
        return np.stack([cf[c].astype(np.float32) for c in "uvp"])[..., None]

    configs = {
        "ldc_quick_double_lid": (inputs("coarse_ldc_Re800_double_lid.h5"), None,
                                 lambda Re: fine.problem(Re, n, n, 1.0, 1.0, 0.001, "QUICK", None, coarse.LDC_DOUBLE_LID)),
        "bfs_upwind_resampled": (inputs("coarse_bfs_Re400.h5"), rs.square_to_rect_resampler(n, n, n, 10.0, 3.0, model.device),
                                 lambda Re: fine.problem(Re, n, n, 10.0, 3.0, 0.002, "UPWIND", None, None,
                                                         bfs={"step_height": 1.0, "h": 2.0, "Ub": 1.0})),
    }
    us = lambda t: round(1e6 * t, 1)
    out = {"mesh": f"{n}x{n}", "warmup": a.warmup, "repeats": a.repeats, "single_only": bool(a.single_only), "handoff": {}}
    for name, (x1, back, make) in configs.items():
        out["handoff"][name] = {}
        for B in [int(b) for b in a.handoff.split(",")]:
            pbs = [make(float(Re)) for Re in np.linspace(100.0, 800.0, B)]
            row = {}
            if not a.single_only:
                x, ain, aout = np.concatenate([x1] * B), np.concatenate([ain1] * B), np.concatenate([aout1] * B)
                b = fine.FineSolverBatch(pbs)
                times = []
                for r in range(a.warmup + a.repeats):
                    t0 = time.perf_counter()
                    b.init_from_prediction(model, x, ain, aout, resampler=back)
                    times.append(time.perf_counter() - t0)
                b.close()
                row["batched_us"] = [us(t) for t in times[a.warmup:]]
                row["batched_us_per_case_median"] = us(float(np.median(times[a.warmup:])) / B)
            solvers = [fine.FineSolver(pb) for pb in pbs]
            times = []
            for r in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                for s in solvers:
                    s.init_from_prediction(model, x1, ain1, aout1, resampler=back)
                times.append(time.perf_counter() - t0)
            for s in solvers:
                s.close()
            row["sequential_single_case_us"] = [us(t) for t in times[a.warmup:]]
            row["sequential_single_case_us_per_case_median"] = us(float(np.median(times[a.warmup:])) / B)
            if not a.single_only:
                row["batched_over_sequential_median"] = round(float(np.median(row["batched_us"]) / np.median(row["sequential_single_case_us"])), 4)
            out["handoff"][name][str(B)] = row
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--batch", default=None, help="comma-separated batch sizes: time the batched solver against sequential solves")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--handoff", default=None, help="comma-separated batch sizes: time the SR hand-off, batched against single-case calls")
    ap.add_argument("--single-only", action="store_true", help="with --handoff: only the single-case calls")
    ap.add_argument("--resident", action="store_true", help="time the resident mode against the launch mode on the meshes of --mesh")
    ap.add_argument("--mesh", default="10,20,30,40,50,64", help="with --resident: comma-separated square mesh sizes")
    ap.add_argument("--pinned", action="store_true", help="with --resident: also the 59 765-iteration 10x10 run in both modes")
    ap.add_argument("--pressure", default=None, choices=("sweeps", "direct"),
                    help="time this inner pressure solver on both configurations at the batch sizes of --batch (default 1,8,16)")
    ap.add_argument("--golden", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"),
                    help="directory of the encoder, statistics and coarse-field files --handoff reads")
    a = ap.parse_args()
    fine = importlib.import_module("sr-for-cfd_amd.fine")
    coarse = importlib.import_module("sr-for-cfd_amd.coarse")
    if a.pressure:
        return pressure_bench(a, fine, coarse)
    if a.resident:
        return resident_bench(a, fine, coarse)
    if a.batch:
        return batch_bench(a, fine, coarse)
    if a.handoff:
        return handoff_bench(a, fine, coarse)
    n = a.n
    configs = {
        "ldc_quick_re1000_double_lid": dict(Re=1000.0, lx=1.0, ly=1.0, dt=0.001, scheme="QUICK", bc=coarse.LDC_DOUBLE_LID, bfs=None),
        "bfs_upwind_re400": dict(Re=400.0, lx=10.0, ly=3.0, dt=0.002, scheme="UPWIND", bc=None, bfs={"step_height": 1.0, "h": 2.0, "Ub": 1.0}),
    }
    out = {"mesh": f"{n}x{n}", "iters": a.iters, "warmup": a.warmup, "floor_us_per_launch": 1.45}
    for name, c in configs.items():
        pb = fine.problem(c["Re"], n, n, c["lx"], c["ly"], c["dt"], c["scheme"], None, c["bc"], bfs=c["bfs"])
        s = fine.FineSolver(pb)
        s.run(a.warmup)
        c0 = s.counters()
        t0 = time.perf_counter()
        s.run(a.iters)
        dt_s = time.perf_counter() - t0
        c1 = s.counters()
        mom = c1["momentum_sweeps"] - c0["momentum_sweeps"]
        prs = c1["pressure_sweeps"] - c0["pressure_sweeps"]
        launches = c1["launches"] - c0["launches"]
        syncs = c1["host_syncs"] - c0["host_syncs"]
        sweep_launches = mom + 2 * prs
        pb_host = fine.problem(c["Re"], n, n, c["lx"], c["ly"], c["dt"], c["scheme"], None, c["bc"], bfs=c["bfs"])
        pb_host.max_iterations = a.host_iters
        L = importlib.import_module("sr-for-cfd_amd._lib")
        import ctypes as C
        var = np.zeros((3, n + 2, n + 2))
        it = C.c_int(0)
        rms = (C.c_double * 3)()
        h0 = time.perf_counter()
        L.check(L.lib.srcfd_coarse_solve(C.byref(pb_host), var.ctypes.data_as(C.c_void_p), C.byref(it), rms))
        host_s = time.perf_counter() - h0
        out[name] = {
            "ms_per_outer_iteration": round(1e3 * dt_s / a.iters, 3),
            "momentum_sweeps_per_solve": round(mom / (2 * a.iters), 1),
            "pressure_sweeps_per_solve": round(prs / a.iters, 1),
            "launches_issued": launches,
            "sweep_launches_executed": sweep_launches,
            "host_syncs": syncs,
            "us_per_sweep_launch": round(1e6 * dt_s / max(1, sweep_launches), 3),
            "host_coarse_solve_ms_per_outer_iteration": round(1e3 * host_s / max(1, it.value), 1),
            "host_over_device": round((host_s / max(1, it.value)) / (dt_s / a.iters), 1),
        }
        s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
