#!/usr/bin/env python3
"""Same kernels, same grids: the launches of two builds of the library, kernel for kernel (profiles/gemm32_plan/).

The template arguments of gemm_mfma_f32<NB, VEC, BKT> are part of the kernel's name, so a kernel trace pins the tile choice that the
output digests of tests/test_gpu_f32_forward_bits.py / test_gpu_train_step_bits.py cannot see.

    SRCFD_LIB=<a libsrcfd.so> rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/gemm32_trace.py run
        every case of the two bits modules once, with plain launches (SRCFD_GRAPH=0, SRCFD_TRAIN_GRAPH=0), in one process
    python3 tools/gemm32_trace.py compare <dir of one build> <dir of the other> <out.json>
        the two sequences of (kernel name, grid size, workgroup size) in dispatch order; exit status 1 if they differ"""
import csv
import glob
import hashlib
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run():
    os.environ["SRCFD_GRAPH"] = "0"
    os.environ["SRCFD_TRAIN_GRAPH"] = "0"
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import conftest
    import srcfd_amd as srcfd
    from oracle import sr_oracle
    fwd = importlib.import_module("test_gpu_f32_forward_bits")
    trn = importlib.import_module("test_gpu_train_step_bits")
    enc = srcfd.SRModel.load_h5(conftest.ENCODER_H5, None, device=-1).weights()
    dec = sr_oracle.synthetic_decoder(1)

    def with_env(env, f):
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return f()
        finally:
            for k, v in saved.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v

    for case in fwd.CASES:
        hr, prec, n, env = case
        m = srcfd.SRModel.from_weights(enc, fwd.decoder_weights(hr), device=0)
        m.precision = prec
        out = np.empty((n, hr, hr, 1), np.float32)
        try:
            with_env(env, lambda: m.predict(fwd.case_input(case), out=out))
            assert m.last_plan()["graph"] == "eager", m.last_plan()
        finally:
            m.close()
        print("forward", fwd.case_id(case), flush=True)
    for case in trn.CASES:
        graph, max_batch, n, env = case
        specs, in_shape, oshape = trn.case_graph(srcfd, enc, dec, graph)
        x, y = trn.case_batch(case, in_shape, oshape)
        Trainer = importlib.import_module("sr-for-cfd_amd.train").Trainer
        t = with_env(env, lambda: Trainer(srcfd.SRModel.from_layers(specs, in_shape, device=0), max_batch=max_batch))   # reads its switches when created
        try:
            t.grads.zero_()
            t.sse.zero_()
            t.forward_backward(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
            torch.cuda.synchronize()
        finally:
            t.close()
        print("train", trn.case_id(case), flush=True)


def launches(directory):
    """[(kernel name, grid, workgroup)] of every kernel_trace.csv under the directory, in dispatch order"""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path, newline="")):
            size = lambda stem: tuple(int(r[k]) for k in sorted(r) if k.startswith(stem))   # ..._X, _Y, _Z
            rows.append((int(r["Dispatch_Id"]), r["Kernel_Name"], size("Grid_Size"), size("Workgroup_Size")))
    rows.sort()
    return [r[1:] for r in rows]


def compare(dir_a, dir_b, out):
    a, b = launches(dir_a), launches(dir_b)
    digest = lambda seq: hashlib.sha256(json.dumps(seq).encode()).hexdigest()
    first = next((i for i, (p, q) in enumerate(zip(a, b)) if p != q), None if len(a) == len(b) else min(len(a), len(b)))
    ours = [x for x in a if "srcfd" in x[0]]
    doc = {"what": "rocprofv3 --kernel-trace of tools/gemm32_trace.py run, once per library; (kernel name, grid size, workgroup size) in dispatch order",
           "launches": [len(a), len(b)], "launches_of_this_library": len(ours),
           "gemm_mfma_instances_seen": sorted({x[0] for x in a if "gemm_mfma" in x[0]}),
           "sha256_of_sequence": [digest(a), digest(b)], "same_multiset": sorted(a) == sorted(b), "equal": a == b,
           "first_difference": None if first is None else {"index": first, "a": a[first] if first < len(a) else None, "b": b[first] if first < len(b) else None}}
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps({k: doc[k] for k in ("launches", "sha256_of_sequence", "same_multiset", "equal", "first_difference")}))
    return 0 if doc["equal"] and a else 1


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["compare"] and len(sys.argv) == 5:
        sys.exit(compare(*sys.argv[2:5]))
    else:
        sys.exit(__doc__)
