"""The 10 -> 400 forward on an MI355X against the integer twins of tests/sr_twins.py, with no tolerance: enc16 -> dense1_16 -> mid16 ->
tail16 / tail16s and every switch arm of them on the scaled encoding (bf16, f16), enc32 / gemm32 / gemm_x3 / the fused f32 chains on
the plain one (fp32, fp32_naive, fp32x3).  test_sr_twins.py proves on the CPU that every intermediate of a twin is an exactly
representable integer whatever the order of a sum, what the encodings mean to the project's own references, and that an index-level
defect in any layer changes the result.

Every comparison is np.array_equal on VALUES (-0 == +0) against the integer model; the non-finite counter must read 0; last_plan()
is asserted for the arm a case is there for.  A mismatch prints the count, the first differing (sample, row, column), the bounding
box and the residues of the differing rows and columns mod 2, 4, 8, 16 (sr_twins.describe_mismatch).

One family of kernels cannot be exact on ANY integer network: the streaming f32 tail (tail32, and its split-operand form under fp32x3)
multiplies ConvT#2's weights and its biases by log2(e) in float32 and the output convolution's by 1 / log2(e), so every product rounds
and the sum over 72 taps depends on its order (sr_twins.py).  A plan whose f32_steps() contain tail32 is therefore held to the integers
after rounding to nearest (every index-level defect moves a value by an integer), and the same arm is run once more under
SRCFD_NO_TAIL32=1, where it is compared exactly.

The batch sizes are the smallest at which each mapping exists (test_gpu_tail16_roles.py): 1 and 3 (pipeline fill and drain), CUs + 3 (a
workgroup walks two samples), SRCFD_TAIL_SEG (segment seams), 130 through predict (the 128-sample staging chunk), 64 and 70 (fp32x3's own
kernels).  The expected fields are computed once per module and shared.
"""
import numpy as np
import pytest

import sr_twins as tw
from conftest import require_gpu

pytestmark = pytest.mark.gpu

SWITCHES = ("SRCFD_ENC", "SRCFD_MID", "SRCFD_MID_WAVES", "SRCFD_MID_ORDER", "SRCFD_DENSE1", "SRCFD_TAIL", "SRCFD_TAIL_SEG", "SRCFD_NO_TAIL32",
            "SRCFD_NO_ENC32", "SRCFD_NO_TRIPLE", "SRCFD_NO_PAIR", "SRCFD_NO_DENSE_SKINNY", "SRCFD_NO_GEMM32_BIG")
DEFAULT16 = dict(encoder="enc16", dense_1="dense1_16", middle="mid16_4x64", tail="tail16")
KINDS16 = ("bf16", "f16")
KINDS32 = ("fp32", "fp32_naive", "fp32x3")


@pytest.fixture(scope="module")
def ctx(srcfd):
    require_gpu(srcfd)
    import torch

    class Ctx:
        pass
    c = Ctx()
    c.torch, c.srcfd = torch, srcfd
    c.cus = torch.cuda.get_device_properties(0).multi_processor_count
    c.twin, c.want, c.t0, c.t1, c.models = {}, {}, {}, {}, {}
    return c


def _twin(ctx, seed):
    """(K, J), the exact output and ConvT#0's / ConvT#1's activations on the 8 samples: once per module, read-only."""
    if seed not in ctx.want:
        K, J = tw.integer_twin(seed)
        y, acts = tw.forward(K, J, tw.inputs(8), return_all=True)
        ctx.twin[seed], ctx.want[seed], ctx.t0[seed], ctx.t1[seed] = (K, J), y, acts[5].astype(np.float32), acts[6].astype(np.float32)
        for a in (ctx.want[seed], ctx.t0[seed], ctx.t1[seed]):
            a.setflags(write=False)
    return ctx.twin[seed]


def _model(ctx, seed, precision):
    encoding = "scaled" if precision in KINDS16 else "plain"
    if (seed, encoding) not in ctx.models:
        ctx.models[(seed, encoding)] = ctx.srcfd.SRModel.from_weights(*tw.encode(*_twin(ctx, seed), encoding), device=0)
    m = ctx.models[(seed, encoding)]
    m.precision = precision
    return m


def _env(monkeypatch, env):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, val)


def _check(got, want, label):
    msg = tw.describe_mismatch(got, want, label)
    assert msg is None, msg


def _forward(ctx, monkeypatch, seed, precision, n, out="float32", affine=True, env=None, host=False):
    """One forward of inputs(n) -> (output as float64 values, the exact expected field, the model).  affine: in_affine on the raw
    input and out_affine, both exact (sr_twins.check_affines); else the integer fields themselves."""
    torch = ctx.torch
    _env(monkeypatch, env or {})
    m = _model(ctx, seed, precision)
    idx = tw.order(n)
    exact = ctx.want[seed][idx]
    ain, raw = tw.in_affine(n)
    aout = tw.out_affine(n)
    x = raw if affine else tw.inputs(n).astype(np.float32)
    if affine:
        exact = tw.apply_out_affine(exact, aout)
    if host:
        assert out == "float32"
        y, bad = m.predict(x, in_affine=ain if affine else None, out_affine=aout if affine else None, nan_guard=True, return_nonfinite=True)
        got = np.array(y, dtype=np.float64)
    else:
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        yd = torch.empty((n, 400, 400, 1), dtype=getattr(torch, out), device="cuda")
        badd = torch.zeros(1, dtype=torch.int64, device="cuda")
        m.predict_device(xd, yd, in_affine=torch.from_numpy(ain).cuda() if affine else None, out_affine=torch.from_numpy(aout).cuda() if affine else None,
                         nan_guard=True, nonfinite=badd)
        torch.cuda.synchronize()
        bad = int(badd.item())
        got = yd.to(torch.float32).cpu().numpy().astype(np.float64)
    assert bad == 0, f"{bad} non-finite values"
    return got, exact, m


def _forward16(ctx, monkeypatch, seed, kind, n, out="float32", affine=True, env=None, host=False, plan=None):
    got, exact, m = _forward(ctx, monkeypatch, seed, kind, n, out, affine, env, host)
    p = m.last_plan()
    want_plan = dict(DEFAULT16, precision=kind, **(plan or {}))
    assert {k: p.get(k) for k in want_plan} == want_plan, p
    _check(got, tw.expected_output(exact, out).astype(np.float64), f"seed {seed} {kind} n = {n} {out}{' affine' if affine else ''} {env or ''}")
    return m


# ------------------------------------------------------------------------------------------------------------------------
# scaled encoding: bf16, f16
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("out", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kind", KINDS16)
def test_default_plan_16bit(ctx, monkeypatch, kind, n, out, affine):
    """float32, bfloat16 and float16 outputs: the exact field rounded to nearest even once.  A float16 output with an out_affine is
    taken on tail16s, whose rounding test_gpu_tail16_roles.py states (one fused v_fma_mixlo_f16); the fma is exact here, so its one
    rounding is the stated one."""
    if out == "float16" and affine:
        _forward16(ctx, monkeypatch, 0, kind, n, out, affine, env={"SRCFD_TAIL": "s"}, plan={"tail": "tail16s"})
    else:
        _forward16(ctx, monkeypatch, 0, kind, n, out, affine)


def _from16(raw, kind):
    return (raw.astype(np.uint32) << 16).view(np.float32) if kind == "bf16" else raw.view(np.float16).astype(np.float32)


ARMS16 = {
    "MID=0": ({"SRCFD_MID": "0"}, {"middle": "gemm16"}),
    "MID=1": ({"SRCFD_MID": "1"}, {"middle": "mid16_8x32"}),
    "MID=2": ({"SRCFD_MID": "2"}, {"middle": "mid16_8x64"}),
    "MID=3": ({"SRCFD_MID": "3"}, {"middle": "mid16_4x64"}),
    "MID_WAVES=4": ({"SRCFD_MID_WAVES": "4"}, {"middle": "mid16_4x32"}),
    "MID_WAVES=16": ({"SRCFD_MID_WAVES": "16"}, {"middle": "mid16_16x32"}),
    "MID_ORDER=1": ({"SRCFD_MID_ORDER": "1"}, {}),
    "TAIL=s": ({"SRCFD_TAIL": "s"}, {"tail": "tail16s"}),
    "TAIL_SEG=1": ({"SRCFD_TAIL_SEG": "1"}, {"tail_seg": "1"}),
    "TAIL_SEG=2": ({"SRCFD_TAIL_SEG": "2"}, {"tail_seg": "2"}),
    "TAIL_SEG=5": ({"SRCFD_TAIL_SEG": "5"}, {"tail_seg": "5"}),
    "TAIL=s,SEG=2": ({"SRCFD_TAIL": "s", "SRCFD_TAIL_SEG": "2"}, {"tail": "tail16s", "tail_seg": "2"}),
    "ENC=0": ({"SRCFD_ENC": "0"}, {"encoder": "layers"}),
    "DENSE1=0": ({"SRCFD_DENSE1": "0"}, {"dense_1": "gemm16"}),
}


@pytest.mark.parametrize("arm", list(ARMS16))
@pytest.mark.parametrize("kind", KINDS16)
def test_switch_arms_16bit(ctx, monkeypatch, kind, arm):
    """Every functional switch of the 16-bit forward at n = 3; in every MID arm ConvT#1's stored activations (and under SRCFD_MID=0
    ConvT#0's) are the twin's integers."""
    env, plan = ARMS16[arm]
    m = _forward16(ctx, monkeypatch, 0, kind, 3, env=env, plan=plan)
    if arm.startswith("MID"):
        idx = tw.order(3)
        _check(_from16(m.debug_activation(0, (3, 50, 50, 64)), kind), ctx.t1[0][idx], f"{kind} {arm} ConvT#1")
        if arm == "MID=0":
            _check(_from16(m.debug_activation(1, (3, 25, 25, 128)), kind), ctx.t0[0][idx], f"{kind} {arm} ConvT#0")


@pytest.mark.parametrize("seg", [None, "1"], ids=["seg=auto", "seg=1"])
@pytest.mark.parametrize("kind", KINDS16)
def test_workgroup_walks_two_samples(ctx, monkeypatch, kind, seg):
    """CUs + 3 samples through predict_device: unsegmented (SRCFD_TAIL_SEG=1) three workgroups run a second sample without draining."""
    _forward16(ctx, monkeypatch, 0, kind, ctx.cus + 3, env={"SRCFD_TAIL_SEG": seg} if seg else None, plan={"tail_seg": seg} if seg else None)


@pytest.mark.parametrize("kind", KINDS16)
def test_staging_chunk_seam_16bit(ctx, monkeypatch, kind):
    """130 samples through predict: the host entry stages 128 samples at a time."""
    _forward16(ctx, monkeypatch, 0, kind, 130, host=True)


@pytest.mark.parametrize("seed", tw.TWIN_SEEDS)
@pytest.mark.parametrize("kind", KINDS16)
def test_every_seed_16bit(ctx, monkeypatch, kind, seed):
    """Together the seeds put a non-zero weight on every MFMA k-step of every layer (test_sr_twins.py::test_reach)."""
    _forward16(ctx, monkeypatch, seed, kind, 1)
    _forward16(ctx, monkeypatch, seed, kind, 1, env={"SRCFD_TAIL": "s"}, plan={"tail": "tail16s"})


# ------------------------------------------------------------------------------------------------------------------------
# plain encoding: fp32, fp32_naive, fp32x3
# ------------------------------------------------------------------------------------------------------------------------
def _forward32(ctx, monkeypatch, seed, precision, n, env=None, host=False, plan=None, affine=True):
    """Exact unless the plan streams the tail through tail32 (module docstring): then equal after rounding to the nearest
    quarter (the out_affine's finest std is 1 / 4), the largest deviation printed.  For the record, an MI355X on 2026-10-21: 4.9e-4 to
    2.0e-3, one float32 ulp of the value, in fp32 and fp32x3 alike."""
    got, exact, m = _forward(ctx, monkeypatch, seed, precision, n, "float32", affine, env, host)
    p = m.last_plan()
    want_plan = dict(precision=precision, **(plan or {}))
    assert {k: p.get(k) for k in want_plan} == want_plan, p
    kernels = [k for _, k, _ in m.f32_steps(n)]
    label = f"seed {seed} {precision} n = {n} {env or ''} {kernels}"
    if "tail32" in kernels:
        assert not (env or {}).get("SRCFD_NO_TAIL32")
        print(f"{label}: tail32 scales by log2(e) in f32; largest deviation from the integers {np.abs(got - exact).max():.3e}")
        _check(np.rint(got * 4), exact * 4, label + " (nearest quarter)")
    else:
        _check(got, exact, label)
    return kernels


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("precision", KINDS32)
def test_default_plan_f32(ctx, monkeypatch, precision, n):
    for affine in (False, True):
        _forward32(ctx, monkeypatch, 0, precision, n, plan={"encoder": "enc32", "dense_1": "dense_skinny32"}, affine=affine)
        kernels = _forward32(ctx, monkeypatch, 0, precision, n, env={"SRCFD_NO_TAIL32": "1"}, affine=affine)
        assert "tail32" not in kernels


@pytest.mark.parametrize("n", [64, 70])
def test_fp32x3_own_kernels(ctx, monkeypatch, n):
    """From 64 samples on fp32x3 runs its split-operand kernels (64: whole tiles; 70: a ragged last tile)."""
    kernels = _forward32(ctx, monkeypatch, 0, "fp32x3", n)
    assert "x3" in kernels, kernels
    kernels = _forward32(ctx, monkeypatch, 0, "fp32x3", n, env={"SRCFD_NO_TAIL32": "1"})
    assert "x3" in kernels and "tail32" not in kernels, kernels


ARMS32 = {
    "NO_TAIL32": ({"SRCFD_NO_TAIL32": "1"}, {}),
    "NO_ENC32": ({"SRCFD_NO_ENC32": "1"}, {"encoder": "layers"}),
    "NO_TRIPLE": ({"SRCFD_NO_TRIPLE": "1"}, {}),
    "NO_PAIR": ({"SRCFD_NO_PAIR": "1"}, {}),
    "NO_DENSE_SKINNY": ({"SRCFD_NO_DENSE_SKINNY": "1"}, {"dense_1": "gemm32"}),
    "NO_GEMM32_BIG": ({"SRCFD_NO_GEMM32_BIG": "1"}, {}),
}


@pytest.mark.parametrize("arm", list(ARMS32))
@pytest.mark.parametrize("precision", KINDS32)
def test_switch_arms_f32(ctx, monkeypatch, precision, arm):
    """One switch at a time at n = 3, and the same switch once more with the layer-by-layer tail, where the comparison is exact."""
    env, plan = ARMS32[arm]
    _forward32(ctx, monkeypatch, 0, precision, 3, env=env, plan=plan)
    if arm != "NO_TAIL32":
        kernels = _forward32(ctx, monkeypatch, 0, precision, 3, env=dict(env, SRCFD_NO_TAIL32="1"), plan=plan)
        assert "tail32" not in kernels


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_staging_chunk_seam_f32(ctx, monkeypatch, precision):
    _forward32(ctx, monkeypatch, 0, precision, 130, env={"SRCFD_NO_TAIL32": "1"}, host=True)


@pytest.mark.parametrize("seed", tw.TWIN_SEEDS)
@pytest.mark.parametrize("precision", KINDS32)
def test_every_seed_f32(ctx, monkeypatch, precision, seed):
    _forward32(ctx, monkeypatch, seed, precision, 1)
    _forward32(ctx, monkeypatch, seed, precision, 1, env={"SRCFD_NO_TAIL32": "1"})
