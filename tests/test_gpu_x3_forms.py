"""Every launch form of the split-bf16 GEMM (csrc/kernels_x3.hip, precision fp32x3) on the device against float64, per element
(tests/x3_forms.py holds the table; tests/test_x3_forms.py proves on a CPU that the table reaches every form and that the statistic
sees one missing product plane, k-tile, sub-block or row).  It mirrors tests/test_gpu_gemm32_forms.py.

For each case: a fresh handle at fp32x3, the output pre-filled with NaN, ONE profiled `predict_device` at the case's batch, the launch
names (exactly one `under_test(x3)`, nothing fused, the front layers under their own names), the engine's step for the layer, and
max_i q_i <= 8 x max(q_cpu, floor) with q_i = |y_i - T_i| / (S_i + |T_i|), gemm32_forms' statistic, bound and MARGIN.  The plan
depends on the CU count, so each case is first asked, through tests/x3_plan_ref.py on the device's own count, whether it still
reaches its tags.  The ratio q / max(q_cpu, floor) of every case is printed; DESIGN.md 4.2d holds the table of a run.

The epilogue's swish, z rcp(1 + exp2(-log2(e) z)), is the chain ACT_BOUND of the f32 file was derived for; it is measured here in the
same way, on an exact GEMM: identity weights are exact under the split (hi carries the 1, and an activation's mid + lo = x - hi is
exact), through the resident and the tiled kernel, z in channel 0 over 64 samples.  Only the finite, normal z are held to the bound:
the split of an infinity is NaN by construction (inf - inf), so for z = +-inf the output is only asserted to be non-finite, which is
what the NaN guard counts; what the bf16 matrix cores return for float32 denormals (whose split is not exact: the packs keep the
high half of the third term) is printed and recorded, not asserted.

The last tests hold the engine to include/srcfd.h's "from 64 samples per call on": the choice between these kernels and the plain f32
ones is made once per call from the caller's n, so a sample's bits do not depend on where the call is cut into chunks or on the
memory type of the destination."""
import ctypes as C
import functools
import importlib
import importlib.util

import numpy as np
import pytest

import gemm32_forms as gf
import x3_forms as xf
from conftest import require_gpu
from test_dropin import page_locked
from test_gpu_gemm32_forms import ACT_BOUND

assert importlib.util.find_spec("pytest_timeout"), "tests/test_gpu_x3_forms.py needs the pytest-timeout plugin for its time limit"
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]   # per test, references included: a hung kernel ends the test


def forward(srcfd, specs, in_shape, x):
    """-> (output, launch names, f32 steps) of one profiled predict_device of a fresh fp32x3 handle"""
    import torch
    m = srcfd.SRModel.from_layers(specs, in_shape, device=0)
    try:
        m.precision = "fp32x3"
        xt = torch.from_numpy(x).cuda()
        yt = torch.full((x.shape[0],) + tuple(m.output_shape), float("nan"), dtype=torch.float32, device="cuda")   # an element nobody writes is a miss
        m.set_profiling(True)
        m.predict_device(xt, yt)
        torch.cuda.synchronize()
        names = [nm for nm, _ in m.get_profile()]
        return yt.cpu().numpy(), names, m.f32_steps(x.shape[0])
    finally:
        m.close()


def identity_spec(channels):
    return [dict(kind="conv2d", k=1, stride=1, same=False, act="swish", name="under_test", w=np.eye(channels, dtype=np.float32).reshape(1, 1, channels, channels),
                 b=np.zeros(channels, np.float32))]


@pytest.fixture(scope="module")
def probe(srcfd, oracle):
    """{kernel: (z, device swish(z), float64 swish(z))} on an exact GEMM"""
    require_gpu(srcfd)
    z = gf.probe_z()
    assert len(z) <= xf.PROBE_N * xf.PROBE_W
    got = {}
    for kernel, channels in (("res", 128), ("tile", 256)):
        assert xf.BY_NAME["probe_" + kernel].in_shape == (1, xf.PROBE_W, channels)   # the graph whose kernel the CPU test proves
        flat = np.zeros(xf.PROBE_N * xf.PROBE_W, np.float32)
        flat[:len(z)] = z
        x = np.zeros((xf.PROBE_N, 1, xf.PROBE_W, channels), np.float32)
        x[..., 0] = flat.reshape(xf.PROBE_N, 1, xf.PROBE_W)   # the other channels stay 0
        y, names, steps = forward(srcfd, identity_spec(channels), (1, xf.PROBE_W, channels), x)
        assert names == ["standardize", "under_test(x3)", "finalize"] and [k for _, k, _ in steps] == ["x3"], (names, steps)
        with np.errstate(over="ignore", invalid="ignore"):
            got[kernel] = (z, y[..., 0].reshape(-1)[:len(z)], oracle._act(z.astype(np.float64), "swish"))
    return got


def normal(z):
    return np.isfinite(z) & ((np.abs(z) >= 2.0 ** -126) | (z == 0))


@pytest.fixture(scope="module")
def activation_error(probe):
    """{activation: the largest |dev - act(z)| / (|z| + |act(z)|) over the finite, normal z and both kernels}, printed"""
    worst = 0.0
    for kernel, (z, y, t) in probe.items():
        ok = normal(z)
        near = np.where(np.abs(y[ok].astype(np.float64) - t[ok]) <= 2.0 ** -150, t[ok], y[ok].astype(np.float64))   # the number format's share, as in the f32 file
        q = gf.q_map(near, t[ok], np.abs(z[ok].astype(np.float64)))
        i = int(np.argmax(q))
        print(f"swish through the x3 {kernel} kernel's epilogue: max q {q.max():.3e} = {q.max() / gf.TINY:.2f} x 2^-24 at z = {z[ok][i]!r}")
        worst = max(worst, float(q.max()))
    return {"swish": worst, "linear": 0.0}


def test_the_swish_epilogue_on_an_exact_gemm(probe, activation_error):
    for kernel, (z, y, t) in probe.items():
        ok = normal(z)
        assert not np.isnan(y[ok]).any(), (kernel, z[ok][np.isnan(y[ok])])
        for zi, yi in zip(z[~np.isfinite(z)], y[~np.isfinite(z)]):
            print(f"x3 {kernel}: z = {zi!r} -> {yi!r}")
            assert not np.isfinite(yi), (kernel, zi, yi)   # inf - inf in the split: NaN by construction, counted by the NaN guard
        for zi, yi, ti in zip(z[np.isfinite(z) & ~ok], y[np.isfinite(z) & ~ok], t[np.isfinite(z) & ~ok]):
            print(f"x3 {kernel}: denormal z = {zi!r} -> {yi!r} (float64 swish {ti!r}); recorded, not asserted")
    assert activation_error["swish"] <= ACT_BOUND, (activation_error, ACT_BOUND)


@functools.lru_cache(maxsize=1)
def reference_of(name):
    case = xf.BY_NAME[name]
    sp, x = gf.specs(case), gf.inputs(case)
    return sp, x, gf.reference(case, sp, x)


@pytest.fixture(scope="module")
def device_plans(srcfd):
    """{case name: the reference's plan of the layer under test on THIS device's CU count}; the descriptors are x3_plan_ref's, which
    tests/test_x3_forms.py holds to the library's own"""
    require_gpu(srcfd)
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {c.name: xf.reference_plan(xf.layer_descriptors(c), cus) for c in xf.CASES}


@pytest.mark.parametrize("name", [c.name for c in xf.CASES])
def test_form_against_float64(srcfd, activation_error, device_plans, name):
    require_gpu(srcfd)
    case = xf.BY_NAME[name]
    got = xf.classify(case, device_plans[name])
    assert set(case.reaches) <= got, f"{name} does not reach {sorted(set(case.reaches) - got)} on {device_plans[name]['cus']} CUs: the table was made for 256"
    sp, x, r = reference_of(name)
    y, names, steps = forward(srcfd, sp, case.in_shape, x)
    # the launches: one forward, the layer under test on its own under its own name, on the split-bf16 kernels
    assert names.count("standardize") == 1 and names.count("under_test(x3)") == 1 and not any("+" in nm for nm in names), names
    assert [nm for nm in names if nm not in ("standardize", "finalize")] == [s["name"] + ("(x3)" if s["name"] == "under_test" else "") for s in sp if "w" in s], names
    mine = [(k, cnt) for nm, k, cnt in steps if nm.split(".ph")[0] == "under_test"]
    assert mine == [("x3", device_plans[name]["count"])], steps
    act = case.layers[-1]["act"]
    assert y.shape == r.T.shape
    qm = gf.q_map(y, r.T, r.S)
    q, at = float(qm.max()), np.unravel_index(int(np.argmax(qm)), r.T.shape)
    floor = gf.bound(0.0, act, activation_error[act]) / gf.MARGIN
    ratio = q / max(r.q_cpu, floor)
    print(f"[{name}] q {q:.3e}, q_cpu {r.q_cpu:.3e}, floor {floor:.3e}, ratio {ratio:.2f} (bar {gf.MARGIN:g}), worst element {tuple(int(v) for v in at)}")
    assert q <= gf.bound(r.q_cpu, act, activation_error[act]), (name, q, r.q_cpu, floor, ratio, at)


# ---------------------------------------------------------------------------------------------------------------------------------
# one decision per call
# ---------------------------------------------------------------------------------------------------------------------------------
SEAM = "tile_same3x3"   # the 64 -> 128 3x3 layer: 8064 output floats per sample


@pytest.fixture(scope="module")
def seam(srcfd):
    """x (150 samples), and y150: one predict_device of all 150 at fp32x3"""
    require_gpu(srcfd)
    import torch
    case = xf.BY_NAME[SEAM]
    sp = gf.specs(case)
    x = np.random.default_rng(150).standard_normal((150,) + case.in_shape).astype(np.float32)
    m = srcfd.SRModel.from_layers(sp, case.in_shape, device=0)
    try:
        m.precision = "fp32x3"
        yt = torch.full((150,) + tuple(m.output_shape), float("nan"), dtype=torch.float32, device="cuda")
        m.predict_device(torch.from_numpy(x).cuda(), yt)
        torch.cuda.synchronize()
        y150 = yt.cpu().numpy()
    finally:
        m.close()
    assert np.isfinite(y150).all()
    return case, sp, x, y150


def x3_names(m):
    return [nm for nm, _ in m.get_profile() if "(x3)" in nm]


def test_a_call_of_150_gives_the_same_bits_into_pageable_and_page_locked_memory_and_on_the_device(srcfd, seam):
    """The host entry cuts a page-locked destination into chunks of 128 and a pageable one into chunks of 256: rows 128 .. 149 are a
    22-sample chunk in the one and part of the only chunk in the other.  The call has 150 samples, so both run the split-bf16 kernels."""
    case, sp, x, y150 = seam
    m = srcfd.SRModel.from_layers(sp, case.in_shape, device=0)
    locked, free_locked = page_locked(y150.shape)
    try:
        m.precision = "fp32x3"
        pageable = np.full(y150.shape, np.nan, np.float32)
        m.predict(x, out=pageable)
        locked[...] = np.nan
        m.set_profiling(True)
        m.predict(x, out=locked)
        last_chunk = x3_names(m)   # the profile is the last chunk's: rows 128 .. 149
        m.set_profiling(False)
        differ = [int(i) for i in np.flatnonzero((locked != y150).any(axis=(1, 2, 3)))]
        assert not differ, f"rows {differ[:3]} .. {differ[-1]} ({len(differ)}) of the page-locked result differ from the device call's"
        np.testing.assert_array_equal(pageable, y150)
        assert last_chunk == ["under_test(x3)"], last_chunk
    finally:
        del locked
        free_locked()
        m.close()


def test_the_remainder_chunk_of_a_device_call_follows_the_call(srcfd, seam):
    """chunk cap + 6 samples through predict_device: the 6-sample remainder runs what the call runs, so every row has the bits of the
    same sample in the 150-sample call"""
    import torch
    case, sp, x, y150 = seam
    m = srcfd.SRModel.from_layers(sp, case.in_shape, device=0)
    try:
        m.precision = "fp32x3"
        L = importlib.import_module("sr-for-cfd_amd._lib")
        cap = L.check(L.lib.srcfd_model_workspace(m._h, 1 << 20, C.byref(C.c_size_t(0))))
        assert 150 < cap <= 1024
        n = cap + 6
        idx = np.arange(n) % 150
        yt = torch.full((n,) + tuple(m.output_shape), float("nan"), dtype=torch.float32, device="cuda")
        m.set_profiling(True)
        m.predict_device(torch.from_numpy(x[idx]).cuda(), yt)
        torch.cuda.synchronize()
        assert x3_names(m) == ["under_test(x3)"] * 2, m.get_profile()   # the whole chunk and the remainder
        y = yt.cpu().numpy()
        differ = [int(i) for i in np.flatnonzero((y != y150[idx]).any(axis=(1, 2, 3)))]
        assert not differ, f"rows {differ[:3]} .. {differ[-1]} ({len(differ)}) differ from the 150-sample call's"
    finally:
        m.close()


def test_a_small_call_after_large_ones_runs_the_plain_f32_kernels(srcfd, seam):
    """Three identical 150-sample calls into a page-locked array (their 22-sample last chunk is captured and replayed as a graph), then
    a call of those 22 samples on their own: below 64 samples per call, so the fp32 path bit for bit, not the graph of the chunk."""
    case, sp, x, y150 = seam
    m = srcfd.SRModel.from_layers(sp, case.in_shape, device=0)
    fresh = srcfd.SRModel.from_layers(sp, case.in_shape, device=0)
    locked, free_locked = page_locked(y150.shape)
    try:
        m.precision = "fp32x3"
        fresh.precision = "fp32"
        want = np.empty((22,) + y150.shape[1:], np.float32)
        fresh.predict(x[128:150], out=want)
        for _ in range(3):
            locked[...] = np.nan
            m.predict(x, out=locked)
            np.testing.assert_array_equal(locked, y150)
        for _ in range(3):   # the small call itself becomes a graph on its second and third run
            np.testing.assert_array_equal(m.predict(x[128:150]), want)
        small = np.empty_like(want)
        m.predict(x[128:150], out=small)
        np.testing.assert_array_equal(small, want)
        m.set_profiling(True)
        np.testing.assert_array_equal(m.predict(x[128:150]), want)
        assert x3_names(m) == [] and "under_test" in [nm for nm, _ in m.get_profile()], m.get_profile()
        assert not np.array_equal(want, y150[128:150])   # the two precisions do differ on these numbers: the comparison can tell them apart
    finally:
        del locked
        free_locked()
        fresh.close()
        m.close()
