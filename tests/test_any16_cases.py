"""CPU companion of test_gpu_any16_layers.py: the case table of tests/any16_cases.py reaches every branch of the generic 16-bit
layer kernels, its integer twins are exact in bf16 and f16 and see every planted geometric defect, the margins of the class
check come from two CPU emulations, and the class check sees local defects at realistic size.  Also the host-side bound on the
16-bit forward's chunk (gemm16's 32-bit offsets).  Nothing here runs on the GPU."""
import importlib

import numpy as np
import pytest

import any16_cases as ac
import error_maps as em
import family_ref as fr
from conftest import STATS_TXT
from test_lowp16_plan import lowp16_plans   # noqa: F401  (the session's one run of the plan harness)


@pytest.fixture(scope="module")
def lr_stats(srcfd):
    return srcfd.load_stats(STATS_TXT, 10, 400)[0]


def test_table_reaches_every_branch_of_the_16bit_layer_kernels():
    """Coverage proof of the table (no GPU): from the specs alone, through the selection rules any16_cases.gemm_ops restates."""
    seen = set()
    for case in ac.CASES:
        h, w = ac.out_hw(case)
        if h != w:
            seen.add("non-square")
        for n in ac.BATCHES + (ac.batch_size(case),):
            ops = ac.gemm_ops(case, n)
            gemms = [d for d in ops if d["kernel"] != "outconv16"]
            seen.add(("outconv16 C", ops[-1]["CI"]))
            assert ops[-1]["kernel"] == "outconv16" and (ops[-1]["MH"], ops[-1]["MW"]) == (h, w)
            if gemms[-1]["M"] % 128 != 0:
                seen.add("last GEMM M % 128 != 0")
            if gemms[-1]["M"] < 32:
                seen.add("last GEMM M < 32")
            for d in ops:
                if d["kernel"] == "gemm16":
                    seen.add(("gemm16 BN", d["BN"]))
                    if d["N"] < d["Npad"]:
                        seen.add("gemm16 N < Npad")
                    if d["Npad"] == 192:
                        seen.add("gemm16 Npad 192")
                if d["kernel"] == "gemm16n":
                    seen.add(("gemm16n CI", d["CI"]))
                    if d["K"] == 16:
                        seen.add("gemm16n one k-step")
                if d["shape"] in ("k2", "k3same", "k3valid"):
                    seen.add((d["kernel"], d["shape"]))
                    seen.add(("ConvT", d["scaling"]))
                if d["shape"] == "out":
                    seen.add(("out", d["scaling"]))
                if d["shape"] == "dense" and d["layer"] != "dense_1":
                    seen.add(("dense behind dense_1", "split-K" if d["splitk"] else "one slab"))
    want = {"non-square", "last GEMM M % 128 != 0", "last GEMM M < 32", "gemm16 N < Npad", "gemm16 Npad 192", "gemm16n one k-step",
            ("gemm16 BN", 64), ("gemm16 BN", 128), ("gemm16n CI", 16), ("gemm16n CI", 32), ("dense behind dense_1", "split-K")}
    want |= {(k, s) for k in ("gemm16", "gemm16n") for s in ("k2", "k3same", "k3valid")}
    want |= {("outconv16 C", c) for c in (16, 32, 48, 64)}
    assert want <= seen, sorted(map(str, want - seen))
    # each of the three weight scalings on a transposed convolution or on the output convolution
    assert {s for kind, s in (t for t in seen if isinstance(t, tuple) and t[0] in ("ConvT", "out"))} == {"q", "q_mul", "q_div"}
    # the phase ops of a 3x3 stride-2 layer: 4 / 2 / 2 / 1 taps; a one-pixel image keeps all four phases
    assert sorted(d["taps"] for d in ac.gemm_ops("narrow16_k3same", 1) if d["shape"] == "k3same") == [1, 2, 2, 4]
    one_px = [d for d in ac.gemm_ops("wide_1px", 1) if d["shape"] == "k3same"]
    assert [(d["MH"], d["MW"]) for d in one_px] == [(1, 1)] * 4
    # ... with one row per sample and K >= 1024, as a Dense layer has: they must not take its split-K branch
    assert [d["K"] for d in one_px] == [2048, 1024, 1024, 512] and not any(d["splitk"] for d in one_px)
    assert {ac.batch_size(c) for c in ac.CASES} == {67, 259} and ac.batch_size("wide_1px") == 259      # 4 corners; one pixel of the % 4 lattice on 4 x 4


def test_gemm_ops_agrees_with_the_library_plan(lowp16_plans):
    """any16_cases.gemm_ops states from a case alone which kernel and branch every op takes; the library's own chunk plan
    (csrc/lowp16_plan.cpp, dumped by the sanitizer-built harness of tests/test_lowp16_plan.py) says the same for every case and
    every batch of BATCHES: kernel, BN, M and whether K is split, op by op, behind enc16 and up to the output convolution."""
    for case in ac.CASES:
        for n in ac.BATCHES:
            steps = lowp16_plans[case]["chunks"][(0, 256, n)]["steps"]      # default switches
            ops = ac.gemm_ops(case, n)
            assert steps[0]["kernel"] == "enc16" and len(steps) == 1 + len(ops), (case, n)
            for st, d in zip(steps[1:], ops):
                assert st["kernel"] == d["kernel"], (case, n, d["layer"])
                if d["kernel"] == "outconv16":
                    assert st["grid"] == (-(-d["M"] // 256),)
                    continue
                assert (st["d"]["M"], st["d"]["N"], st["d"]["K"], st["d"]["Npad"], st["d"]["CI"]) == (d["M"], d["N"], d["K"], d["Npad"], d["CI"]), (case, n, d["layer"])
                if d["kernel"] == "gemm16n":
                    assert d["BN"] == 32 and st["grid"] == (-(-d["M"] // 128), d["Npad"] // d["BN"]) and not d["splitk"], (case, n, d["layer"])
                else:
                    assert st["cut"]["bn"] == d["BN"] and (st["cut"]["splits"] > 1) == d["splitk"], (case, n, d["layer"])


def test_every_case_is_accepted_on_a_host_only_handle(srcfd, enc_weights):
    for case in ac.CASES:
        for weights, lin in ((ac.random_decoder(case), False), (ac.integer_twin(case, 0), True)):
            m = srcfd.SRModel.from_layers(ac.build_specs(case, enc_weights, weights, all_linear=lin), (10, 10, 1), device=-1)
            assert m.output_shape == ac.out_hw(case) + (1,)
            assert m.supports_precision("bf16") and m.supports_precision("f16") and not m.has_fused_path, case
            assert m.footprint(3, "bf16")["device_workspace"] > 0


# ------------------------------------------------------------------------------------------------------------------------
# B. the integer twins
# ------------------------------------------------------------------------------------------------------------------------
def test_integer_twins_are_exact_in_both_16bit_formats(enc_weights, coarse_cases, lr_stats):
    """The proof that test_gpu_any16_layers.py may ask for bit equality: on every twin the 16-bit emulation (weights and every
    activation handed on rounded to bf16 / f16) IS the float64 forward, so every intermediate is representable; the plain integer
    restatement twin_reference agrees, and no activation passes 256 in magnitude.  Over the seeds of a case every tap and every
    input channel of the output convolution is read."""
    x = em.fixed_batch(coarse_cases, lr_stats, 3)
    for case in ac.CASES:
        taps, chans = np.zeros((3, 3), bool), None
        for seed in ac.TWIN_SEEDS:
            weights = ac.integer_twin(case, seed)
            specs = ac.build_specs(case, enc_weights, weights, all_linear=True)
            y64 = fr.forward_specs64(specs, x)
            assert y64.shape == (3,) + ac.out_hw(case) + (1,) and np.abs(y64).max() > 0
            for kind in ac.KINDS:
                np.testing.assert_array_equal(fr.forward_specs_lowp(specs, x, kind), y64, err_msg=f"{case} seed {seed} {kind}")
            y, peak = ac.twin_reference(case, weights)
            assert peak <= 256, (case, seed, peak)
            for i in range(3):
                np.testing.assert_array_equal(y64[i, ..., 0], y.astype(np.float64), err_msg=f"{case} seed {seed}")
            wo = weights["output_image"][0][..., 0] != 0
            assert 2 <= wo.sum() <= 16          # a handful
            taps |= wo.any(2)
            chans = wo.any((0, 1)) if chans is None else chans | wo.any((0, 1))
        assert taps.all() and chans.all(), (case, taps, chans)


def test_every_planted_geometry_defect_changes_the_twin():
    """One defect at a time in the numpy restatement, in every transposed convolution of every case it applies to: at least one
    output element of at least one seed moves (so a device with that defect fails the bit-for-bit test)."""
    applied = {d: 0 for d in ac.TWIN_DEFECTS}
    for case in ac.CASES:
        for layer in range(len(ac.CASES[case]["convts"])):
            for defect in ac.TWIN_DEFECTS:
                if not ac.defect_applies(case, defect, layer):
                    continue
                moved = 0
                for seed in ac.TWIN_SEEDS:
                    weights = ac.integer_twin(case, seed)
                    good, _ = ac.twin_reference(case, weights)
                    bad, _ = ac.twin_reference(case, weights, defect, layer)
                    moved += int((good != bad).sum()) if good.shape == bad.shape else good.size
                assert moved > 0, (case, layer, defect)
                applied[defect] += 1
    assert all(applied[d] >= 3 for d in ac.TWIN_DEFECTS), applied


# ------------------------------------------------------------------------------------------------------------------------
# C. position classes and their margins
# ------------------------------------------------------------------------------------------------------------------------
def test_grid_classes_follow_the_geometry():
    cl = em.grid_classes(5, 6, 10, stacked=2, sample_group=2)
    assert all(m.shape == (5, 6, 10) for m in cl.values())
    for mod in (2, 4):          # every lattice and the sample groups are partitions
        assert (sum(cl[k].astype(int) for k in cl if k.startswith(f"lattice/row%{mod}")) == 1).all()
    assert (sum(cl[k].astype(int) for k in cl if k.startswith("sample/")) == 1).all()
    assert [k for k in cl if k.startswith("sample/")] == ["sample/0-1", "sample/2-4"]           # the remainder joins the last group
    assert sorted(k for k in cl if k.startswith("border/")) == sorted(f"border/{a}_{i}" for a, n in (("row", 6), ("col", 10)) for i in (0, 1, n - 2, n - 1))
    assert cl["corner/all_four"].sum() == 4 * 5 and cl["single/row_3"].sum() == 10 * 5 and cl["single/col_9"].sum() == 6 * 5
    assert sum(k.startswith("single/") for k in cl) == 16
    assert not any("%4" in k for k in em.grid_classes(1, 4, 4, stacked=1))
    assert sorted(k for k in em.grid_classes(1, 5, 7, pool=2) if k.startswith("single/row")) == ["single/row_0-1", "single/row_2-3", "single/row_4-4"]
    assert list(em.grid_classes(3, 4, 4, sample_group=16))[-1] == "sample/0-2"


def _second(case, kind, ref):
    return fr.forward_specs_lowp2(ref["specs"], ref["x"], kind)[..., 0]


def test_spreads_are_calibrated_on_two_emulations(enc_weights, coarse_cases, lr_stats):
    """spread = max over the case's classes of rms_C(E' - T) / rms_C(E - T), and for the worst single element; none may exceed the
    figure any16_cases.SPREAD carries for its kind, which is what the GPU module's margin (2 x) is built on.  No margin above 4.
    E' in the device's place passes the class check and the per-sample bounds of the GPU module."""
    from test_gpu_parity_bf16 import MEDIAN_EMU, TOL, per_sample_rel_l2
    for case in ac.CASES:
        ref = ac.references(case, enc_weights, coarse_cases, lr_stats)
        assert all(m.sum() >= 256 for kind in ac.KINDS for m in ref["classes"][kind].values()), case
        for kind in ac.KINDS:
            E2 = _second(case, kind, ref)
            s, at, elem = em.spread((E2 - ref["T"])[None], (ref[kind] - ref["T"])[None], ref["classes"][kind])
            e = per_sample_rel_l2(E2, ref[kind])
            print(f"{case:18s} {kind:4s} n = {ac.batch_size(case)}: spread {s:.4f} ({at}) | {elem:.4f}; E' vs E per sample max {e.max():.2e} median {np.median(e):.2e}")
            assert max(s, elem) <= ac.SPREAD[kind], (case, kind, s, at, elem)
            ok, report, _, _ = em.class_check((E2 - ref["T"])[None], (ref[kind] - ref["T"])[None], ref["classes"][kind], 2 * ac.SPREAD[kind], f"{case} {kind} E'")
            assert ok, report
            assert e.max() <= TOL[kind][0] and np.median(e) <= MEDIAN_EMU[kind]
    assert all(2 * v <= 4.0 for v in ac.SPREAD.values())


def test_local_defects_at_realistic_size_fail_the_class_check(enc_weights, coarse_cases, lr_stats):
    """The emulation E stands in for the device, with one defect of the size a kernel's edge handling produces: the last row
    computed without one tap of the output convolution, the same on one corner pixel alone, and the pixels of output phase (0, 1)
    holding their left neighbours' values (phase (0, 0)).  The class check must fail and name the class among its ten worst."""
    for case in ac.CASES:
        ref = ac.references(case, enc_weights, coarse_cases, lr_stats)
        H, W = ac.out_hw(case)
        specs = ref["specs"]
        wo = np.array(specs[-1]["w"])
        wo[0, 1] = 0                                   # the tap above the pixel
        no_tap = specs[:-1] + [dict(specs[-1], w=wo)]
        for kind in ac.KINDS:
            E, T = ref[kind], ref["T"]
            E_tap = fr.forward_specs_lowp(no_tap, ref["x"], kind)[..., 0]
            row, corner, phase = E.copy(), E.copy(), E.copy()
            row[:, H - 1] = E_tap[:, H - 1]
            corner[:, H - 1, W - 1] = E_tap[:, H - 1, W - 1]
            phase[:, 0::2, 1::2] = E[:, 0::2, 0:2 * (W // 2):2]
            planted = {"last row without one tap": (row, {f"border/row_{H - 1}", f"single/row_{H - 1}"}),
                       "one corner pixel without one tap": (corner, {"corner/all_four"}),
                       "phase (0, 1) holds phase (0, 0)": (phase, {"lattice/row%2==0,col%2==1"})}
            for name, (y, expect) in planted.items():
                ok, report, ten, worst = em.class_check((y - T)[None], (E - T)[None], ref["classes"][kind], 2 * ac.SPREAD[kind], f"{case} {kind} {name}")
                assert not ok, report
                assert expect & set(ten), f"planted class not among the ten worst\n{report}"


# ------------------------------------------------------------------------------------------------------------------------
# D. gemm16 forms element offsets in 32-bit int: a chunk never holds 2^31 activation elements
# ------------------------------------------------------------------------------------------------------------------------
def _workspace(chunk, max_act):
    """lowp16_workspace_bytes: two 16-bit activation buffers + 16 split-K slabs of (chunk x 128) f32."""
    return 2 * chunk * max_act * 2 + 16 * chunk * 128 * 4


def test_a_16bit_chunk_stays_below_2_to_31_activation_elements(srcfd, enc_weights):
    """An accepted graph whose largest activation is 1024 x 1024 x 16 = 2^24 elements per sample (eight 2x2 transposed
    convolutions from 4 x 4): 1024 samples per chunk would be 2^34 elements, and gemm16's `xoff` / `off` are int.  The chunk is
    127 samples, 127 x 2^24 < 2^31, read off footprint()'s device workspace on a host-only handle (nothing is allocated or run).
    The five family decoders keep 1024 samples per chunk and the footprint they had."""
    rng = np.random.default_rng(31)
    fam = importlib.import_module("sr-for-cfd_amd.family")
    u = lambda *shape: rng.uniform(-0.1, 0.1, shape).astype(np.float32)
    specs = fam.encoder_specs(enc_weights, 10) + [dict(kind="dense", name="dense_1", act="swish", w=u(50, 1024), b=u(1024)),
                                                  dict(kind="reshape", name="reshape", shape=(4, 4, 64))]
    cin = 64
    for i in range(8):
        specs.append(dict(kind="conv2d_transpose", name=f"up{i}", k=2, stride=2, same=False, act="swish", w=u(2, 2, 16, cin), b=u(16)))
        cin = 16
    specs.append(dict(kind="conv2d", name="out", k=3, stride=1, same=True, act="linear", w=u(3, 3, 16, 1), b=u(1)))
    m = srcfd.SRModel.from_layers(specs, (10, 10, 1), device=-1)
    assert m.output_shape == (1024, 1024, 1) and m.supports_precision("bf16")
    max_act = 1024 * 1024 * 16
    cap = (2 ** 31 - 1) // max_act
    assert cap == 127 and cap * max_act < 2 ** 31 <= (cap + 1) * max_act
    for kind in ac.KINDS:
        for n, chunk in ((1, 1), (100, 100), (127, 127), (128, 127), (1024, 127), (5000, 127)):
            assert m.footprint(n, kind)["device_workspace"] == _workspace(chunk, max_act), (kind, n)
    # the family: largest activation = the last transposed convolution's output (conv2d_1's 3200 elements are less everywhere)
    for hr in (10, 20, 50, 80, 100):
        (h, w, c), convts = fam.DECODER_CONVTS[hr]
        acts = [3200, h * w * c]
        for f, k, same in convts:
            h, w = fam.convt_out(h, k, 2, same), fam.convt_out(w, k, 2, same)
            acts.append(h * w * f)
        fm = srcfd.SRModel.from_weights(enc_weights, fam.synthetic_decoder_weights(hr, seed=1), device=-1)
        for n in (1, 6, 1024, 1030, 5000):
            assert fm.footprint(n, "bf16")["device_workspace"] == _workspace(min(n, 1024), max(acts)), (hr, n)
