"""The training step (csrc/train.hip: trainer_build, trainer_step) bit for bit against tests/golden/train_step_digests.json,
recorded by tests/golden/record_train_step.py on the commit that file names.  The kernels, their launch parameters and the order
of every float addition are the recorded commit's, so the host code that plans the weight-gradient launches, the slab sums and
the buffer sizes may be reorganised freely and no gradient bit moves.  A case is one fresh Trainer and four calls -- plain
launches, the call that is captured, the replayed graph, and an overwriting call over NaN-filled buffers -- which must all give
the recorded sha256 of the flat gradient and the recorded bits of the squared-error sum.  An undersized split-K workspace is
refused (csrc/gemm32_plan.h, gemm32_ws_fits) and an undersized slab space loses slabs, so the digests pin the sizing too.  An intended
change of a training kernel's arithmetic re-records the file and says so."""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, require_gpu

pytestmark = pytest.mark.gpu

RECORDED_ON = "a1f0ad2"   # the last commit whose step planned its weight-gradient launches and slab sums inside the launch loop
LAYERWISE = {"SRCFD_TRAIN_TAIL": "0", "SRCFD_TRAIN_ENC": "0"}
# (graph, max_batch, samples, switches)
CASES = [
    ("sr", 8, 1, {}),            # both fusions: ten ops + the fused tail's slabs in the table
    ("sr", 8, 5, {}),
    ("sr", 8, 8, {}),
    ("sr", 8, 4, LAYERWISE),     # all 14 ops, ConvT#0's four phases sharing a bias; ConvT#4's slab count peaks at 4 and 8 samples ...
    ("sr", 8, 5, LAYERWISE),     # ... and falls in between
    ("sr", 8, 5, {"SRCFD_TRAIN_FUSE": "0"}),
    ("sr", 8, 5, {"SRCFD_TRAIN_OVERLAP": "0"}),
    ("sr", 8, 5, {"SRCFD_TRAIN_GRAPH": "0"}),
    ("sr", 7, 4, {"SRCFD_TRAIN_TAIL": "0"}),   # the batch whose slab need exceeds max_batch's own
    ("convt_3s2", 3, 3, {}),     # four phases of 4 / 2 / 2 / 1 taps
    ("dense_reshape_conv", 3, 3, {}),
    ("tail_6x7", 8, 3, {}),      # the fused tail on a 6 x 7 image
]
GOLDEN_JSON = os.path.join(GOLDEN, "train_step_digests.json")
CALLS = ("plain", "capture", "replay", "overwrite")


def case_id(case):
    graph, max_batch, n, env = case
    return "-".join([graph, f"max{max_batch}", f"n{n}"] + [f"{k}={v}" for k, v in env.items()])


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def case_graph(srcfd, enc_weights, dec_weights, graph):
    """-> (layer specs, input shape, output shape) of a case's graph"""
    orc = importlib.import_module("test_gpu_training_oracle")
    if graph == "sr":
        return srcfd.layers_from_weights(enc_weights, dec_weights), (10, 10, 1), (400, 400, 1)
    if graph == "tail_6x7":
        return orc._tail_specs(6, 7)[0], (6, 7, 3), (48, 56, 1)
    specs, in_shape = orc.TABLE[graph][:2]
    return specs, in_shape, orc.out_shape(specs, in_shape)


def case_batch(case, in_shape, oshape):
    graph, max_batch, n, env = case
    rng = np.random.default_rng(7000 + 10 * n + len(graph))   # the switches of a graph and batch share their input
    return rng.standard_normal((n,) + tuple(in_shape)).astype(np.float32), rng.standard_normal((n,) + tuple(oshape)).astype(np.float32)


def run_case(srcfd, enc_weights, dec_weights, case):
    """-> (sha256 of x, y and the initial parameters, [(sha256 of grads, bits of sse as hex)] of the four CALLS)"""
    import torch
    graph, max_batch, n, env = case
    specs, in_shape, oshape = case_graph(srcfd, enc_weights, dec_weights, graph)
    x, y = case_batch(case, in_shape, oshape)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)   # the trainer reads its switches when it is created
    try:
        t = importlib.import_module("sr-for-cfd_amd.train").Trainer(srcfd.SRModel.from_layers(specs, in_shape, device=0), max_batch=max_batch)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        want_plan = {"fused_tail": int(graph in ("sr", "tail_6x7") and env.get("SRCFD_TRAIN_TAIL") != "0"),
                     "fused_encoder": int(graph == "sr" and env.get("SRCFD_TRAIN_ENC") != "0")}
        assert t.plan == want_plan, (case_id(case), t.plan)
        inputs = sha256(x, y, t.params.cpu().numpy())
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        got = []
        for call in CALLS:
            if call == "overwrite":
                t.grads.fill_(float("nan"))
                t.sse.fill_(float("nan"))
            else:
                t.grads.zero_()
                t.sse.zero_()
            t.forward_backward(xd, yd, overwrite=call == "overwrite")
            torch.cuda.synchronize()
            got.append((sha256(t.grads.cpu().numpy()), t.sse.cpu().numpy().tobytes().hex()))
        return inputs, got
    finally:
        t.close()


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_train_step_has_the_recorded_bits(srcfd, enc_weights, dec_weights, case):
    require_gpu(srcfd)
    doc = json.load(open(GOLDEN_JSON))
    assert doc["commit"] == RECORDED_ON, "re-recorded: name the new commit here, in the commit that changes a training kernel's arithmetic"
    assert sorted(doc["cases"]) == sorted(case_id(c) for c in CASES)
    golden = doc["cases"][case_id(case)]
    inputs, got = run_case(srcfd, enc_weights, dec_weights, case)
    print(case_id(case), inputs, got)
    assert inputs == golden["input_sha256"], "the generators' draws or the initial parameters changed, not the step"
    for call, (grads, sse) in zip(CALLS, got):
        assert grads == golden["grads_sha256"], f"{call}: gradient bits differ from commit {doc['commit']}'s"
        assert sse == golden["sse_bits"], f"{call}: the squared-error sum's bits differ from commit {doc['commit']}'s"
