"""BASELINE config 5 (40x40x3 -> 1600x1600x3 through 4x4 tiles, f16), one process: the host path against the device path.

Arms, alternating call by call, 3 warm-up rounds, then median [min - max] of 20 rounds:
  a  pipeline.tiled_super_resolution, numpy in / numpy out (the existing path)
  b  pipeline.tiled_super_resolution_device, numpy in / numpy out
  c  the same, tensor in / tensor out, HIP events on the stream
  d  the stitch kernel alone, HIP events, with its bytes/s beside the 6.29 TB/s copy figure; once with `out` as allocated (the plan
     picks V = 4) and with `out` 8 and 4 bytes off that alignment (V = 2, V = 1): the evidence for the plan's choice of V.  The
     three take turns at going first (whoever follows another stitch finds y in the memory-side cache).  The same at 16x16 tiles
     (768 samples, 2 x 491 MB), where the kernel runs long enough for the rate to mean something.
  o  the overlapped path, 34x34x3 with overlap 2: 4x4 tiles and 48 samples, the network work of config 5, a 1360x1360x3 result --
     o_b numpy in / numpy out, o_c tensor in / tensor out (HIP events), o_d the blending stitch alone (HIP events) with its
     bytes/s (all 48 planes read, the result written) beside the copy figure.  The host function with the same overlap is run
     once, for the bit-for-bit check, and not timed.
Prints one JSON object; --out writes it to a file as well.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.29e12     # measured float4 copy rate of the MI355X, bytes/s (read + write)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-overlapped", action="store_true", help="arms a - d only: the loop of this tool before it had the overlapped arms")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sr-for-cfd_amd")
    pl = importlib.import_module("sr-for-cfd_amd.pipeline")
    synth = importlib.import_module("sr-for-cfd_amd.synth")
    golden = os.path.join(ROOT, "tests", "golden")
    enc_w = pkg.SRModel.load_h5(os.path.join(golden, "vanilla_encoder10_to_400_swish_trained_upto_700_multiBC.h5"), None, device=-1).weights()
    model = pkg.SRModel.from_weights(enc_w, synth.synthetic_decoder_weights(1), device=0)
    model.precision = args.precision
    ty = tx = 4
    C = 3
    field = np.random.default_rng(5).standard_normal((ty * 10, tx * 10, C)).astype(np.float32)
    f_dev = torch.from_numpy(field).cuda()
    out_dev = torch.empty((ty * 400, tx * 400, C), dtype=torch.float32, device="cuda")
    tiler = pkg.Tiler(model, ty, tx, C)
    n = tiler.n
    y_dev = torch.randn((n, 400, 400), dtype=torch.float32, device="cuda")

    def stitch_targets(t):
        """`out` of tiler t inside one allocation, at the three alignments that make the plan pick V = 4, 2, 1"""
        size = int(np.prod(t.out_shape))
        pad = torch.empty(size + 4, dtype=torch.float32, device="cuda")
        o = {v: pad[k:k + size].view(t.out_shape) for v, k in ((4, 0), (2, 2), (1, 1))}
        for v, x in o.items():
            assert t.plan(align_bytes=16 if v == 4 else 4 * v)["v"] == v and x.data_ptr() % (4 * v) == 0 and (v == 4 or x.data_ptr() % (8 * v))
        return o
    outs = stitch_targets(tiler)
    big = pkg.Tiler(model, 16, 16, C)
    y_big = torch.randn((big.n, 400, 400), dtype=torch.float32, device="cuda")
    outs_big = stitch_targets(big)
    overlap = 2
    field_o = np.random.default_rng(6).standard_normal((ty * (10 - overlap) + overlap, tx * (10 - overlap) + overlap, C)).astype(np.float32)
    fo_dev = torch.from_numpy(field_o).cuda()
    tiler_o = pkg.Tiler(model, ty, tx, C, overlap=overlap)
    out_o = torch.empty(tiler_o.out_shape, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()

    def timed_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    def timed_wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        dt = (time.perf_counter() - t0) * 1e3
        return dt, r

    arms = {k: [] for k in ("a", "b", "c", "d_v4", "d_v2", "d_v1", "big_v4", "big_v2", "big_v1", "o_b", "o_c", "o_d")}
    same = None
    want_o = pl.tiled_super_resolution(field_o, model, 10, overlap=overlap)
    same_o = None
    for it in range(args.warmup + args.rounds):
        ta, ya = timed_wall(lambda: pl.tiled_super_resolution(field, model, 10))
        tb, yb = timed_wall(lambda: pl.tiled_super_resolution_device(field, model, 10))
        tc = timed_events(lambda: pl.tiled_super_resolution_device(f_dev, model, 10, out=out_dev))
        order = [(4, 2, 1), (2, 1, 4), (1, 4, 2)][it % 3]
        td = {v: timed_events(lambda: tiler.stitch(y_dev, outs[v])) for v in order}
        tbig = {v: timed_events(lambda: big.stitch(y_big, outs_big[v])) for v in order}
        if not args.skip_overlapped:
            tob, yob = timed_wall(lambda: pl.tiled_super_resolution_device(field_o, model, 10, overlap=overlap))
            toc = timed_events(lambda: pl.tiled_super_resolution_device(fo_dev, model, 10, out=out_o, overlap=overlap))
            if same_o is None:
                same_o = bool(np.array_equal(want_o.view(np.uint32), yob.view(np.uint32)) and np.array_equal(want_o.view(np.uint32), out_o.cpu().numpy().view(np.uint32)))
            del yob
            tod = timed_events(lambda: tiler_o.stitch(y_dev, out_o))
        if it >= args.warmup and not args.skip_overlapped:
            arms["o_b"].append(tob)
            arms["o_c"].append(toc)
            arms["o_d"].append(tod)
        if same is None:
            same = bool(np.array_equal(ya.view(np.uint32), yb.view(np.uint32)) and np.array_equal(ya.view(np.uint32), out_dev.cpu().numpy().view(np.uint32)))
        del ya, yb
        if it >= args.warmup:
            arms["a"].append(ta)
            arms["b"].append(tb)
            arms["c"].append(tc)
            for v in (4, 2, 1):
                arms[f"d_v{v}"].append(td[v])
                arms[f"big_v{v}"].append(tbig[v])
    stitch_bytes = 2 * out_dev.numel() * 4
    rec = {"workload": "BASELINE config 5: 40x40x3 -> 1600x1600x3 via 4x4 tiles, 48 samples", "precision": args.precision, "warmup": args.warmup,
           "arms": {"a_host_path_numpy": summary(arms["a"]), "b_device_path_numpy": summary(arms["b"]), "c_device_path_tensor_events": summary(arms["c"])},
           "stitch_alone": {}, "stitch_alone_768_samples": {}, "stitch_bytes": stitch_bytes, "copy_rate_bytes_per_s": COPY_RATE, "stitch_floor_ms_at_copy_rate": round(stitch_bytes / COPY_RATE * 1e3, 4),
           "device_equals_host_bit_for_bit": same, "plan": tiler.plan(), "device": torch.cuda.get_device_name(0)}
    for v in (4, 2, 1):
        s = summary(arms[f"d_v{v}"])
        s["bytes_per_s_at_median"] = round(stitch_bytes / (s["median_ms"] * 1e-3))
        s["fraction_of_copy_rate"] = round(s["bytes_per_s_at_median"] / COPY_RATE, 3)
        rec["stitch_alone"][f"v{v}"] = s
        s = summary(arms[f"big_v{v}"])
        s["bytes_per_s_at_median"] = round(16 * stitch_bytes / (s["median_ms"] * 1e-3))
        s["fraction_of_copy_rate"] = round(s["bytes_per_s_at_median"] / COPY_RATE, 3)
        rec["stitch_alone_768_samples"][f"v{v}"] = s
    if not args.skip_overlapped:
        blend_bytes = (y_dev.numel() + out_o.numel()) * 4
        sd = summary(arms["o_d"])
        sd["bytes"] = blend_bytes
        sd["bytes_per_s_at_median"] = round(blend_bytes / (sd["median_ms"] * 1e-3))
        sd["fraction_of_copy_rate"] = round(sd["bytes_per_s_at_median"] / COPY_RATE, 3)
        rec["overlapped"] = {"workload": f"34x34x3 -> 1360x1360x3 via 4x4 tiles of 10x10 with overlap {overlap}, 48 samples", "b_device_path_numpy": summary(arms["o_b"]),
                             "c_device_path_tensor_events": summary(arms["o_c"]), "d_blending_stitch_alone": sd, "device_equals_host_bit_for_bit": same_o,
                             "plan": tiler_o.plan()}
    a = rec["arms"]["a_host_path_numpy"]
    rec["bar"] = {"b_median_below_a_range": a["min_ms"] > rec["arms"]["b_device_path_numpy"]["median_ms"],
                  "c_median_below_a_range": a["min_ms"] > rec["arms"]["c_device_path_tensor_events"]["median_ms"]}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
