"""The two 16-bit forwards (fused_bf16.hip: the encoder_10 + decoder_400 graph and the other family graphs) bit for bit against
tests/golden/lowp16_output_digests.json, recorded by tests/golden/record_lowp16_outputs.py on the commit that file names.  The
kernels and their launch parameters are the recorded commit's, so host code between the launches may be reorganised freely and
these bits do not move: every arm of the shared encoder front and GEMM chain (enc16 or layer by layer, dense1_16 or gemm16, mid16
or gemm16, gemm16n) is reached by one case.  An intended change of a kernel's arithmetic re-records the file and says so."""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, require_gpu

pytestmark = pytest.mark.gpu

RECORDED_ON = "7d44389"   # the last commit with two separate 16-bit forwards: the parent of the one that shared their front end
FUSED = {"encoder": "enc16", "dense_1": "dense1_16", "middle": "mid16_4x64", "tail": "tail16"}
ANY16 = {"encoder": "enc16", "decoder": "any16"}
# (decoder, samples, switches, what last_plan() must say).  decoder_400 at n = 3 is the small call (tail segmentation > 1); its
# three switched cases run the generic layer loop; decoder_80 is the graph whose narrow-channel GEMM runs.
GRAPHS = [
    (400, 3, {}, FUSED),
    (400, 7, {}, FUSED),
    (400, 3, {"SRCFD_ENC": "0"}, dict(FUSED, encoder="layers")),
    (400, 3, {"SRCFD_DENSE1": "0"}, dict(FUSED, dense_1="gemm16")),
    (400, 3, {"SRCFD_MID": "0"}, dict(FUSED, middle="gemm16")),
    (10, 6, {}, ANY16),
    (80, 6, {}, ANY16),
    (80, 6, {"SRCFD_ENC": "0"}, dict(ANY16, encoder="layers")),
]
CASES = [(hr, n, env, plan, kind) for hr, n, env, plan in GRAPHS for kind in ("bf16", "f16")]


def case_id(case):
    hr, n, env, _, kind = case
    return "-".join([f"decoder_{hr}", f"n{n}"] + [f"{k}={v}" for k, v in env.items()] + [kind])


def case_input(case):
    hr, n, env, _, kind = case
    seed = 1000 * hr + 10 * n + len(env)   # the two operand types of a case share their input
    return np.random.default_rng(seed).standard_normal((n, 10, 10, 1)).astype(np.float32)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(srcfd, enc_weights, case, predicts=1):
    """-> (outputs of `predicts` identical calls, last_plan() of the last one)"""
    hr, n, env, _, kind = case
    if hr == 400:
        dec = importlib.import_module("sr-for-cfd_amd.synth").synthetic_decoder_weights(1)
    else:
        dec = importlib.import_module("sr-for-cfd_amd.family").synthetic_decoder_weights(hr)
    m = srcfd.SRModel.from_weights(enc_weights, dec, device=0)
    m.precision = kind
    x = case_input(case)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ys = [m.predict(x) for _ in range(predicts)]
        plan = m.last_plan()
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        m.close()
    return ys, plan


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_16bit_forward_has_the_recorded_bits(srcfd, enc_weights, case):
    require_gpu(srcfd)
    hr, n, env, want_plan, kind = case
    doc = json.load(open(os.path.join(GOLDEN, "lowp16_output_digests.json")))
    assert doc["commit"] == RECORDED_ON, "re-recorded: name the new commit here, in the commit that changes a 16-bit kernel's arithmetic"
    assert sorted(doc["cases"]) == sorted(case_id(c) for c in CASES)
    golden = doc["cases"][case_id(case)]
    assert sha256(case_input(case)) == golden["input_sha256"], "the generator's draws changed, not the engine"
    ys, plan = run_case(srcfd, enc_weights, case, predicts=2)
    assert plan["precision"] == kind and {k: plan.get(k) for k in want_plan} == want_plan, plan
    if hr == 400 and n == 3:
        assert int(plan["tail_seg"]) > 1, plan
    for i, y in enumerate(ys):
        assert y.shape == (n, hr, hr, 1) and y.dtype == np.float32
        assert sha256(y) == golden["output_sha256"], f"call {i}: output bits differ from commit {doc['commit']}'s"
