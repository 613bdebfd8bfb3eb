"""The f32-grade forward (engine.hip, forward_generic: SRCFD_PREC_FP32, FP32X3, FP32_NAIVE) bit for bit, and launch for launch,
against tests/golden/f32_forward_digests.json, recorded by tests/golden/record_f32_forward.py on the commit that file names.  The
kernels and their launch parameters are the recorded commit's, so the host code that chooses them may be reorganised freely and
neither the bits nor the list of launch names move: every arm of the choice (enc32 or layer by layer, dense_skinny32, the grouped
and single generic GEMMs with split-K, gemm32_big, the split-bf16 GEMMs, tail32 / triple / pair / every layer on its own,
gemm_finalize, the bring-up kernels) is reached by one case.  An intended change of a kernel's arithmetic re-records the file and
says so.  The second test is about a handle's history: what a handle reserved or predicted before must not change what it computes."""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, require_gpu

pytestmark = pytest.mark.gpu

RECORDED_ON = "cbb7d7b"   # the last commit whose f32 forward chose its kernels inside the launch loop: the parent of the one with the step resolver
NO_TAIL32 = {"SRCFD_NO_TAIL32": "1"}
# (decoder, precision, samples, switches)
CASES = [
    (400, "fp32", 3, {}),      # enc32, dense_skinny32, ConvT#0's phases as one generic launch with split-K, gemm_mfma, tail32
    (400, "fp32", 7, {}),
    (400, "fp32", 216, {}),    # gemm32_big: ConvT#0's phases as one launch, ConvT#1 on its own
    (400, "fp32", 216, {"SRCFD_NO_GEMM32_BIG": "1"}),   # the same size on the generic kernels
    (400, "fp32", 3, {"SRCFD_NO_ENC32": "1"}),          # layer-by-layer encoder
    (400, "fp32", 3, {"SRCFD_NO_DENSE_SKINNY": "1"}),   # generic dense_1
    (400, "fp32", 3, NO_TAIL32),                        # convt_triple + gemm_finalize
    (400, "fp32", 3, dict(NO_TAIL32, SRCFD_NO_TRIPLE="1")),   # convt_pair
    (400, "fp32", 3, dict(NO_TAIL32, SRCFD_NO_PAIR="1")),     # every layer materialised
    (400, "fp32x3", 63, {}),   # below the split-bf16 threshold: the fp32 path
    (400, "fp32x3", 64, {}),   # at it
    (400, "fp32_naive", 3, {}),
    (10, "fp32", 6, {}),       # the family's padding='same' transposed convolutions and last-layer kernels
    (80, "fp32", 6, {}),
    (100, "fp32", 6, {}),
    (80, "fp32x3", 64, {}),
]
GOLDEN_JSON = os.path.join(GOLDEN, "f32_forward_digests.json")


def case_id(case):
    hr, prec, n, env = case
    return "-".join([f"decoder_{hr}", prec, f"n{n}"] + [f"{k}={v}" for k, v in env.items()])


def case_input(case):
    hr, prec, n, env = case
    seed = 1000 * hr + 10 * n + len(env)   # the precisions of a graph and batch share their input
    return np.random.default_rng(seed).standard_normal((n, 10, 10, 1)).astype(np.float32)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def decoder_weights(hr):
    if hr == 400:
        return importlib.import_module("sr-for-cfd_amd.synth").synthetic_decoder_weights(1)
    return importlib.import_module("sr-for-cfd_amd.family").synthetic_decoder_weights(hr)


def predict_profiled(m, x, out, predicts=3):
    """-> (sha256 of each of `predicts` identical calls, last_plan() after each, launch names of one more call).  The result goes
    into the caller's pageable array, so a call is one forward of up to 256 samples; the names are taken on a call of their own
    because profiling switches graph replay off."""
    shas, plans = [], []
    for _ in range(predicts):
        m.predict(x, out=out)
        shas.append(sha256(out))
        plans.append(m.last_plan())
    m.set_profiling(True)
    m.predict(x, out=out)
    names = [name for name, _ in m.get_profile()]
    m.set_profiling(False)
    assert sha256(out) == shas[0], "the profiled call computes other bits"
    return shas, plans, names


def run_case(srcfd, enc_weights, case):
    hr, prec, n, env = case
    m = srcfd.SRModel.from_weights(enc_weights, decoder_weights(hr), device=0)
    m.precision = prec
    x = case_input(case)
    out = np.empty((n, hr, hr, 1), np.float32)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return predict_profiled(m, x, out)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        m.close()


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_f32_forward_has_the_recorded_bits_and_launches(srcfd, enc_weights, case):
    require_gpu(srcfd)
    hr, prec, n, env = case
    doc = json.load(open(GOLDEN_JSON))
    assert doc["commit"] == RECORDED_ON, "re-recorded: name the new commit here, in the commit that changes an f32 kernel's arithmetic"
    assert sorted(doc["cases"]) == sorted(case_id(c) for c in CASES)
    golden = doc["cases"][case_id(case)]
    assert sha256(case_input(case)) == golden["input_sha256"], "the generator's draws changed, not the engine"
    shas, plans, names = run_case(srcfd, enc_weights, case)
    print(case_id(case), shas, plans, names)
    want_graph = ["eager", "capture", "replay"] if n <= 96 else ["eager"] * 3
    assert [p["graph"] for p in plans] == want_graph, plans
    for i, (sha, plan) in enumerate(zip(shas, plans)):
        assert sha == golden["output_sha256"], f"call {i} ({plan['graph']}): output bits differ from commit {doc['commit']}'s"
        assert dict(plan, graph="") == dict(golden["plan"], graph=""), (plan, golden["plan"])
    assert names == golden["launches"], "the launches differ from the recorded commit's"
    x3_launches = [nm for nm in names if "(x3)" in nm]
    assert bool(x3_launches) == (prec == "fp32x3" and n >= 64), names
    if prec == "fp32x3" and n < 64:   # below the threshold the call IS the fp32 path: same kernels, same bits
        as_fp32 = run_case(srcfd, enc_weights, (hr, "fp32", n, env))
        assert as_fp32[0] == shas and as_fp32[2] == names


@pytest.mark.parametrize("reserve,n", [(256, 32), (768, 100), (768, 160)])
def test_a_handles_history_does_not_change_its_bits(srcfd, enc_weights, reserve, n):
    """reserve(256) sizes the split-K slabs for a batch whose ConvT#0 runs on gemm32_big, which needs none; a later smaller call on
    that handle runs ConvT#0 on the generic kernels, which do.  It must compute what a fresh handle computes, with the same
    launches.  On the recorded commit the slab was sized by the first call alone (conv2d_1's 12 800 floats per reserved sample):
    at (256, 32) and (768, 100) ConvT#0's phases then ran as four launches instead of one, each still fitting its own slabs into
    it, so the bits held; at (768, 160) the 4 x 169-pixel phase no longer fit (13.8 M floats against 9.8 M), ran unsplit and
    summed in another order."""
    require_gpu(srcfd)
    x = np.random.default_rng(400 + reserve + n).standard_normal((n, 10, 10, 1)).astype(np.float32)
    out = np.empty((n, 400, 400, 1), np.float32)
    got = []
    for first in (0, reserve):
        m = srcfd.SRModel.from_weights(enc_weights, decoder_weights(400), device=0)
        try:
            if first:
                m.reserve(first)
            shas, plans, names = predict_profiled(m, x, out, predicts=1)
        finally:
            m.close()
        print(f"reserve({first}) then n = {n}:", shas[0], names)
        got.append((shas[0], names))
    assert got[1][1] == got[0][1], "launches differ after reserve"
    assert got[1][0] == got[0][0], f"predict({n}) after reserve({reserve}) differs in bits from a fresh handle's"
