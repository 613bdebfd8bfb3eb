"""Every launch form of the f32 GEMM on the device against float64, per element (tests/gemm32_forms.py holds the table, the statistic
and its argument; tests/test_gemm32_forms.py proves on a CPU that the table reaches every form).

For each case: the model at fp32, ONE profiled `predict_device` at the case's batch (one forward: the table keeps every batch inside
one chunk), the launch names (the layer under test went out under its own name, nothing fused took it, no split-bf16 kernel), the
engine's step for it under the case's switches, and max_i q_i <= 8 x max(q_cpu, floor) with q_i = |y_i - T_i| / (S_i + |T_i|).
The ratio q / max(q_cpu, floor) of every case is printed; DESIGN.md 4.2d holds the table of a run.

The activations are measured apart from the sums (`activation_error`): a 1x1 convolution with identity weights and zero bias is an
exact GEMM, so what it returns for z is the device's act(z).  Over [-100, 100], the edges of float32's exponent range, zeros,
denormals and infinities, through the mfma epilogue and through conv_n1_f32's, the error is held to ACT_BOUND and then added to the
floor of the nonlinear cases.  ACT_BOUND = 8 x 2^-24 of |z| + |act(z)|: swish is v * rcp(1 + exp2(-log2(e) v)), three IEEE roundings of
2^-24 and two hardware functions that kernels_fp32.hip gives as <= 2 ulp = 2^-22 each; relative to act(z) that is at most
(|v| (1 - sigmoid) + 4) 2^-24 from the exponential, 2^-24 from the sum, 4 x 2^-24 from the reciprocal and 2^-24 from the product, and
act(z) is at most half of |z| + |act(z)|, |v| sigmoid (1 - sigmoid) / (1 + sigmoid) at most 1/4: 5.25 x 2^-24, rounded up.  The sigmoid is the
same chain without the last product, tanhf is a library function of a few ulp of a result below 1; relu and linear are exact."""
import contextlib
import functools
import importlib.util
import os

import numpy as np
import pytest

import gemm32_forms as gf
from conftest import require_gpu

assert importlib.util.find_spec("pytest_timeout"), "tests/test_gpu_gemm32_forms.py needs the pytest-timeout plugin for its time limit"
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]   # per test, references included: a hung kernel ends the test
ACT_BOUND = 8 * gf.TINY


@contextlib.contextmanager
def environment(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def forward(srcfd, specs, in_shape, x, env=None):
    """-> (output, launch names, f32 steps, last_plan) of one profiled predict_device of a fresh fp32 handle"""
    import torch
    with environment(env or {}):
        m = srcfd.SRModel.from_layers(specs, in_shape, device=0)
        try:
            m.precision = "fp32"
            xt = torch.from_numpy(x).cuda()
            yt = torch.full((x.shape[0],) + tuple(m.output_shape), float("nan"), dtype=torch.float32, device="cuda")   # an element nobody writes is a miss
            m.set_profiling(True)
            m.predict_device(xt, yt)
            torch.cuda.synchronize()
            names = [nm for nm, _ in m.get_profile()]
            return yt.cpu().numpy(), names, m.f32_steps(x.shape[0]), m.last_plan()
        finally:
            m.close()


def identity_spec(channels, act):
    return [dict(kind="conv2d", k=1, stride=1, same=False, act=act, name="under_test", w=np.eye(channels, dtype=np.float32).reshape(1, 1, channels, channels),
                 b=np.zeros(channels, np.float32))]


@pytest.fixture(scope="module")
def probe(srcfd, oracle):
    """{(epilogue, activation): (z, device act(z), float64 act(z))} on an exact GEMM"""
    require_gpu(srcfd)
    z = gf.probe_z()
    got = {}
    for epi, channels in (("mfma", 2), ("n1", 1)):
        assert gf.BY_NAME["probe_" + epi].in_shape == (1, len(z), channels)   # the graph whose route the CPU test proves
        x = np.zeros((1, 1, len(z), channels), np.float32)
        x[0, 0, :, 0] = z   # the other channel stays 0: inf x 0 would spoil only the column that is not read
        for act in gf.ACTS:
            y, names, _, _ = forward(srcfd, identity_spec(channels, act), (1, len(z), channels), x)
            assert names == ["standardize", "under_test", "finalize"], names
            with np.errstate(over="ignore", invalid="ignore"):
                got[epi, act] = (z, y[0, 0, :, 0], oracle._act(z.astype(np.float64), act))
    return got


@pytest.fixture(scope="module")
def activation_error(probe):
    """{activation: the largest |dev - act(z)| / (|z| + |act(z)|) over finite z and both epilogues}, printed"""
    worst = {a: 0.0 for a in gf.ACTS}
    for (epi, act), (z, y, t) in probe.items():
        fin = np.isfinite(z)
        # float32 cannot come closer to act(z) than half its smallest denormal, 2^-150 (swish(2^-149) = 2^-150 rounds to 0): that much of
        # the difference is the number format's, not the activation's
        near = np.where(np.abs(y[fin].astype(np.float64) - t[fin]) <= 2.0 ** -150, t[fin], y[fin].astype(np.float64))
        q = gf.q_map(near, t[fin], np.abs(z[fin].astype(np.float64)))
        i = int(np.argmax(q))
        print(f"activation {act} through the {epi} epilogue: max q {q.max():.3e} = {q.max() / gf.TINY:.2f} x 2^-24 at z = {z[fin][i]!r}")
        worst[act] = max(worst[act], float(q.max()))
    return worst


def test_the_activations_on_an_exact_gemm(probe, activation_error):
    """The measured term, and kernels_fp32.hip's claims about the ends as assertions: swish(-inf) = -0, swish(+inf) = +inf, no NaN
    for finite z; every activation meets float64 exactly at +-inf."""
    for (epi, act), (z, y, t) in probe.items():
        fin = np.isfinite(z)
        assert not np.isnan(y[fin]).any(), (epi, act, z[fin][np.isnan(y[fin])])
        for zi, yi, ti in zip(z[~fin], y[~fin], t[~fin]):
            assert act == "swish" or yi == np.float32(ti), (epi, act, zi, yi, ti)   # swish: below (the oracle's own silu(-inf) is inf x 0)
        if act == "swish":
            neg = y[z == -np.inf]
            assert neg.size == 1 and neg[0] == 0 and np.signbit(neg[0]) and y[z == np.inf][0] == np.inf, (epi, y[~fin])
        if act in ("linear", "relu"):
            assert np.array_equal(y[fin], t[fin].astype(np.float32)), (epi, act)   # the GEMM in front is exact, denormals included
    for act, e in activation_error.items():
        assert e <= (0.0 if act in ("linear", "relu") else ACT_BOUND), (act, e, ACT_BOUND)


@functools.lru_cache(maxsize=2)
def reference_of(base):
    """specs, inputs and reference of a case, shared by the arms of its switch (they follow each other in the table)"""
    case = gf.BY_NAME[base]
    sp, x = gf.specs(case), gf.inputs(case)
    return sp, x, gf.reference(case, sp, x)


def expected_step(case):
    for tag in case.reaches:
        if tag.startswith("step:"):
            w = tag.split(":")
            return w[1], int(w[2]) if len(w) > 2 else None
    return None


@pytest.mark.parametrize("name", [c.name for c in gf.CASES])
def test_form_against_float64(srcfd, activation_error, name):
    require_gpu(srcfd)
    case = gf.BY_NAME[name]
    sp, x, r = reference_of(name.split("_off")[0])
    y, names, steps, plan = forward(srcfd, sp, case.in_shape, x, case.env)
    # the launches: one forward, the layer under test on its own under its own name
    assert names.count("standardize") == 1 and names.count("under_test") == 1 and not any("+" in nm or "(x3)" in nm for nm in names), names
    assert [nm for nm in names if nm not in ("standardize", "finalize")] == [s["name"] for s in sp if "w" in s], names
    mine = [(k, cnt) for nm, k, cnt in steps if nm.split(".ph")[0] == "under_test"]
    assert len(mine) == 1 and mine[0][0] in ("mfma", "group", "finalize", "big", "skinny"), steps
    want = expected_step(case)
    if want:   # the pre-empting kernels and their switches: the choice the launch loop made under this environment
        assert mine[0][0] == want[0] and want[1] in (None, mine[0][1]), (steps, want)
        assert plan["dense_1"] == ("gemm32" if case.env.get("SRCFD_NO_DENSE_SKINNY") == "1" else "dense_skinny32"), plan
    act = case.layers[-1]["act"]
    assert y.shape == r.T.shape
    q = gf.statistic(y, r.T, r.S)
    floor = gf.bound(0.0, act, activation_error[act]) / gf.MARGIN
    ratio = q / max(r.q_cpu, floor)
    print(f"[{name}] {mine[0][0]}: q {q:.3e}, q_cpu {r.q_cpu:.3e}, floor {floor:.3e}, ratio {ratio:.2f} (bar {gf.MARGIN:g})")
    assert q <= gf.bound(r.q_cpu, act, activation_error[act]), (name, q, r.q_cpu, floor, ratio, np.unravel_index(int(np.argmax(gf.q_map(y, r.T, r.S))), r.T.shape))
