"""Host-buffer SRModel.predict (numpy in / out) on encoder_10 + decoder_400: the PCIe + pageable-memory inclusive rate.

    python tools/host_predict_bench.py                     bf16 and fp32 at 3 / 48 / 768 samples, best of 5 calls, as text
    python tools/host_predict_bench.py --small-call 200    the host-bound call alone: 3 samples, bf16, into a reused array; one JSON
                                                           line with the median / min / max ms of that many calls after 20 warm-up
                                                           calls (the figure of profiles/lowp16_host/)
    python tools/host_predict_bench.py --small-call 300 --precision fp32    the same call on the f32 path (profiles/f32_plan/, profiles/gemm32_plan/)"""
import argparse, importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--small-call", type=int, default=0, metavar="CALLS")
ap.add_argument("--precision", default="bf16", help="of --small-call")
args = ap.parse_args()
srcfd = importlib.import_module('sr-for-cfd_amd'); synth = importlib.import_module('sr-for-cfd_amd.synth')
enc = srcfd.SRModel.load_h5(os.path.join(ROOT, 'tests/golden/vanilla_encoder10_to_400_swish_trained_upto_700_multiBC.h5'), None, device=-1).weights()
m = srcfd.SRModel.from_weights(enc, synth.synthetic_decoder_weights(1), device=0)
if args.small_call:
    m.precision = args.precision
    x = np.random.default_rng(0).standard_normal((3, 10, 10, 1)).astype(np.float32)
    y = m.predict(x)
    for _ in range(20): m.predict(x, out=y)
    t = []
    for _ in range(args.small_call):
        t0 = time.perf_counter(); m.predict(x, out=y); t.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"n": 3, "precision": args.precision, "calls": len(t), "median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t), "plan": m.last_plan()}))
    sys.exit(0)
for prec in ("bf16", "fp32"):
    m.precision = prec
    for n in (3, 48, 768):
        x = np.random.default_rng(0).standard_normal((n, 10, 10, 1)).astype(np.float32)
        m.predict(x)
        t = []
        for _ in range(5):
            t0 = time.perf_counter(); y = m.predict(x); t.append(time.perf_counter() - t0)
        dt = min(t)
        print(f"{prec} host predict n={n}: {dt*1e3:.2f} ms -> {n/3/dt:.0f} fields/s, {y.nbytes/dt/1e9:.1f} GB/s out")
        t = []
        for _ in range(5):
            t0 = time.perf_counter(); m.predict(x, out=y); t.append(time.perf_counter() - t0)
        dt = min(t)
        print(f"{prec} host predict n={n} into a reused array: {dt*1e3:.2f} ms -> {n/3/dt:.0f} fields/s, {y.nbytes/dt/1e9:.1f} GB/s out")
