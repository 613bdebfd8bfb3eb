"""Times the device scorer (EvalSet.score, csrc/score.hip) and prints one JSON line per leg.  Not a test.

    python tools/score_bench.py --leg score   [--samples 6,96,768] [--precisions fp32,bf16] [--repeats 7] [--warmup 2]
    python tools/score_bench.py --leg kernel  [--samples 768] [--repeats 5]
    python tools/score_bench.py --leg fit     [--train-samples 96] [--val-samples 6] [--repeats 5]

--leg score: per sample count and precision, the wall time of one EvalSet.score call (forward of the resident set in chunks of
256, score kernel, n x 8 floats back; ends in a host synchronisation) against the host loop `train_main.evaluate_for_re` runs on
the same samples and the same handle: one `predict` per sample, the 640 kB field back to the host, numpy reductions.  400 x 400
fields (encoder_10 + synthetic decoder_400), 6 = the notebook's held-out set.  The two alternate inside every repeat; the
medians, the ranges and the device's clocks before and after the leg are reported, and whether MAE has the same bits both ways.

--leg kernel: EvalSet.score on `--samples` 400 x 400 fields, bf16 forward, repeated; meant to run under
`rocprofv3 --kernel-trace --stats` (kernel time of score_fields_kernel: three launches of 256 samples for 768) and, in a run
of its own, under `rocprofv3 --pmc ...`.  Prints the traffic floor: two reads of samples x 160 000 x 4 bytes at 6.3 TB/s.

--leg fit: what a user picks `validation_every` from: one `train.validate` (export_model + score + close) on `--val-samples`
held-out 400 x 400 samples against one training epoch (`fit(epochs=1)`, batch 8) on `--train-samples`; also export_model alone.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12   # achievable HBM rate of the MI355X (float4 copy)


def _stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": [round(x, 4) for x in v]}


def _clocks():
    import bench
    import torch
    try:
        pr = torch.cuda.get_device_properties(0)
        pci = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
    except Exception:   # noqa: BLE001
        pci = None
    return bench.gpu_state(pci)


def _model(srcfd):
    synth = importlib.import_module("sr-for-cfd_amd.synth")
    enc = srcfd.SRModel.load_h5(os.path.join(ROOT, "tests", "golden", "vanilla_encoder10_to_400_swish_trained_upto_700_multiBC.h5"), None, device=-1).weights()
    return srcfd.SRModel.from_weights(enc, synth.synthetic_decoder_weights(1), device=0)


def _data(n, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 10, 10, 1)).astype(np.float32)
    truth = np.empty((n, 400, 400, 1), np.float32)
    for i in range(n):
        truth[i] = rng.standard_normal((400, 400, 1), dtype=np.float32)
    comps = np.array(["u", "v", "p"] * (n // 3 + 1))[:n]
    stats = {"u": (0.02, 0.23), "v": (-0.01, 0.11), "p": (0.003, 0.04)}
    return x, truth, comps, stats


def leg_score(a, srcfd):
    tm = importlib.import_module("sr-for-cfd_amd.train_main")
    ds = importlib.import_module("sr-for-cfd_amd.datasets")
    model = _model(srcfd)
    out = {"leg": "score", "field": "400x400", "repeats": a.repeats, "warmup": a.warmup, "clocks_before": _clocks(), "cases": []}
    for n in a.samples:
        x, truth, comps, stats = _data(n)
        data = dict(x_lr_test=x, x_hr_test=truth, res_test=np.full(n, 800), comps_test=comps, stats_hr=stats)
        es = ds.evalset_from_split(data, 800)
        for prec in a.precisions:
            model.precision = prec
            dev_ms, host_ms = [], []
            for r in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                got = es.score(model)
                t1 = time.perf_counter()
                ref = tm.evaluate_for_re(800, model, data, 400)
                t2 = time.perf_counter()
                if r >= a.warmup:
                    dev_ms.append((t1 - t0) * 1e3)
                    host_ms.append((t2 - t1) * 1e3)
            # evaluate_for_re predicts one sample per call, EvalSet.score up to 256: the forward picks its kernels by the sample count, so
            # the bits agree only where both take the same kernels
            same = [float(m) == r_ for m, r_ in zip(got["mae"], ref["mae"])]
            out["cases"].append({"samples": n, "precision": prec, "evalset_score_ms": _stats(dev_ms), "evaluate_for_re_ms": _stats(host_ms),
                                 "speedup_median": float(np.median(host_ms) / np.median(dev_ms)), "mae_bits_equal_to_one_sample_predicts": f"{sum(same)}/{n}",
                                 "plan": model.last_plan()})
        es.close()
    out["clocks_after"] = _clocks()
    print(json.dumps(out), flush=True)


def leg_kernel(a, srcfd):
    model = _model(srcfd)
    model.precision = "bf16"
    n = a.samples[0]
    x, truth, comps, stats = _data(n)
    aff = np.array([stats[c] for c in comps], np.float32)
    es = srcfd.EvalSet(x, truth, pred_affine=aff, truth_affine=aff)
    ms = []
    for r in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        es.score(model)
        if r >= a.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    bytes_read = 2 * n * 160000 * 4
    print(json.dumps({"leg": "kernel", "samples": n, "field": "400x400", "score_calls": a.warmup + a.repeats, "evalset_score_ms": _stats(ms),
                      "score_kernel_bytes_read": bytes_read, "traffic_floor_us_at_6.3TBps": bytes_read / HBM_BYTES_PER_S * 1e6,
                      "note": "kernel time: sum of the score_fields_kernel launches of one call in the rocprofv3 kernel trace of this run"}), flush=True)
    es.close()


def leg_fit(a, srcfd):
    import torch
    tr = importlib.import_module("sr-for-cfd_amd.train")
    synth = importlib.import_module("sr-for-cfd_amd.synth")
    enc, dec = synth.keras_default_init(0)
    trainer = tr.Trainer(srcfd.SRModel.from_weights(enc, dec, device=0), max_batch=8)
    xl, xh, _, _ = _data(a.train_samples, seed=1)
    vx, vt, comps, stats = _data(a.val_samples, seed=2)
    aff = np.array([stats[c] for c in comps], np.float32)
    es = srcfd.EvalSet(vx, vt, pred_affine=aff, truth_affine=aff)
    out = {"leg": "fit", "train_samples": a.train_samples, "val_samples": a.val_samples, "batch_size": 8, "clocks_before": _clocks()}
    epoch_ms, val_ms, export_ms = [], [], []
    for r in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        tr.fit(trainer, xl, xh, epochs=1, batch_size=8, seed=r)   # includes the upload of the training arrays, as every fit call does
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        tr.validate(trainer, es, r + 1)
        t2 = time.perf_counter()
        m = trainer.export_model()
        t3 = time.perf_counter()
        m.close()
        if r >= a.warmup:
            epoch_ms.append((t1 - t0) * 1e3)
            val_ms.append((t2 - t1) * 1e3)
            export_ms.append((t3 - t2) * 1e3)
    out.update(fit_one_epoch_ms=_stats(epoch_ms), validate_ms=_stats(val_ms), export_model_ms=_stats(export_ms),
               validate_over_epoch=float(np.median(val_ms) / np.median(epoch_ms)), clocks_after=_clocks())
    print(json.dumps(out), flush=True)
    es.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["score", "kernel", "fit"], required=True)
    ap.add_argument("--samples", default=None)
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--train-samples", type=int, default=96)
    ap.add_argument("--val-samples", type=int, default=6)
    a = ap.parse_args()
    a.samples = [int(s) for s in (a.samples or ("768" if a.leg == "kernel" else "6,96,768")).split(",")]
    a.precisions = a.precisions.split(",")
    srcfd = importlib.import_module("sr-for-cfd_amd")
    if srcfd.device_count() < 1:
        raise SystemExit("score_bench needs a HIP device: there is nothing to time without one")
    {"score": leg_score, "kernel": leg_kernel, "fit": leg_fit}[a.leg](a, srcfd)


if __name__ == "__main__":
    main()
