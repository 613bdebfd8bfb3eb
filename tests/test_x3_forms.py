"""The table of split-bf16 GEMM launch forms (tests/x3_forms.py) on a CPU: that every case reaches the form it is in the table for and
that the table reaches every form, proved from the library's own plan of the table's graphs -- tools/pack_digest.cpp --forms, the
sanitizer-built harness, dumps plan_gemm_x3's answer (csrc/x3_plan.cpp, on 256 CUs) for every layer the kernels take, and
srcfd_model_f32_steps of a host-only handle at fp32x3 says which kernel the engine's launch loop would send each layer to -- that
every dumped line is what tests/x3_plan_ref.py, the launchers' rules as they stood before the plan was factored out of them, gives,
and that the per-element statistic of tests/test_gpu_x3_forms.py rejects, on each case's own numbers, one small product of the six
left out of the whole layer, one 32-deep k-tile left out of one element, one 32-channel sub-block taken from the neighbouring phase
and one output row taken from the next pixel, while it accepts a float32 emulation of the kernels' own arithmetic.  A case that
stops reaching its form fails here, without a GPU."""
import functools

import numpy as np
import pytest

import family_ref
import gemm32_forms as gf
import x3_forms as xf
import x3_plan_ref as ref
from conftest import ROOT


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return xf.dump_plans(tmp_path_factory.mktemp("x3_forms"), ROOT)


@pytest.fixture(scope="module")
def steps(srcfd):
    """{case name: (kernel, ops) of the layer under test}: the engine's own choice on a host-only handle at fp32x3"""
    got = {}
    for c in xf.CASES:
        m = srcfd.SRModel.from_layers(gf.specs(c), c.in_shape, device=-1)
        try:
            m.precision = "fp32x3"
            st = m.f32_steps(c.batch)
            small = m.f32_steps(63)
        finally:
            m.close()
        assert all(k not in ("enc32", "tail32", "triple", "pair") for _, k, _ in st), (c.name, st)   # nothing fused swallows a layer
        assert all(k != "x3" for _, k, _ in small), (c.name, small)                                   # a call below 64 samples: the plain f32 kernels
        assert all(k != "x3" for name, k, _ in st if name.split(".ph")[0] != "under_test"), (c.name, st)   # a front layer is not on these kernels
        mine = [(k, cnt) for name, k, cnt in st if name.split(".ph")[0] == "under_test"]
        assert len(mine) == 1, (c.name, st)
        got[c.name] = mine[0]
    return got


def test_the_dump_holds_the_table(plans):
    assert list(plans) == [c.name for c in xf.CASES]
    for c in xf.CASES:
        assert [g["layer"] for g in plans[c.name]] == [len(c.layers) - 1], c.name   # the layer under test and no front layer
        g = plans[c.name][0]
        assert g["cus"] == 256 and all(o["d"]["M"] == c.batch * o["d"]["MH"] * o["d"]["MW"] and ref.qualifies(o["d"]) for o in g["ops"]), c.name
        assert [o["d"] for o in g["ops"]] == xf.layer_descriptors(c), c.name   # the descriptors the device test plans from are the library's


def test_every_line_matches_the_reference(plans):
    """grouped or not, the group's grid and its table of first workgroups, every op's kernel, weight row length, own grid and tile
    count, on the dump's 256 CUs and on CU counts the dump does not have"""
    for name, (g,) in plans.items():
        ds = [o["d"] for o in g["ops"]]
        want = xf.reference_plan(ds, g["cus"])
        for key in ("count", "grouped", "group_grid", "first5"):
            assert g[key] == want[key], (name, key, g[key], want[key])
        for got, w in zip(g["ops"], want["ops"]):
            for key in ("kernel", "kpad", "grid", "ntiles", "res"):
                assert got[key] == w[key], (name, key, got[key], w[key])
            assert got["kpad"] == got["d"]["K"] and got["kpad"] % ref.BK == 0   # CI % 32 == 0: no padded k
        if g["grouped"]:   # the table the kernel decodes: op i owns [first[i], first[i + 1]), rows x column blocks each, in the ops' order
            sizes = [ref.ceil_div(d["M"], ref.BP) * (d["N"] // ref.BN) for d in ds]
            assert list(np.diff(g["first5"][:len(ds) + 1])) == sizes and g["first5"][0] == 0 and g["group_grid"] == sum(sizes), name


def test_each_case_reaches_the_form_it_names_and_the_table_reaches_every_form(plans, steps):
    reached = set()
    for c in xf.CASES:
        g = plans[c.name][0]
        assert steps[c.name] == ("x3", g["count"]), (c.name, steps[c.name])   # one x3 step takes the layer, all its phases
        got = xf.classify(c, g)
        assert set(c.reaches) <= got, (c.name, sorted(set(c.reaches) - got), sorted(got))
        assert xf.classify(c, xf.reference_plan([o["d"] for o in g["ops"]], g["cus"])) == got, c.name   # what the device test asks on its own CU count
        reached |= set(c.reaches)
    assert not xf.WANT - reached, sorted(xf.WANT - reached)
    # both activations on each kernel, a linear case on each
    assert {xf.BY_NAME[n].reaches[0].split(":")[0] for n in xf.LINEAR_CASES} >= {"tile", "group", "res"}


def test_the_table_stays_small(plans):
    """Spatial sizes of a few pixels; nothing above the second-tile case's 8.5 M output floats; one forward per call."""
    for c in xf.CASES:
        ops = plans[c.name][0]["ops"]
        out = c.batch * ops[0]["d"]["OH"] * ops[0]["d"]["OW"] * ops[0]["d"]["OC"]
        flops = sum(2 * o["d"]["M"] * o["d"]["N"] * o["d"]["K"] for o in ops)
        assert out <= 8.6e6 and flops <= 2.2e9 and 64 <= c.batch <= 70, (c.name, out, flops)
        assert c.name == "res_second_tile" or max(c.in_shape[:2]) <= 10 or c.name.startswith("probe"), c.name


# ---------------------------------------------------------------------------------------------------------------------------------
# the statistic on each case's own numbers
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def numbers(name):
    case = xf.BY_NAME[name]
    sp, x = gf.specs(case), gf.inputs(case)
    r = gf.reference(case, sp, x)
    h = gf.layer_input64(sp, x).astype(np.float32)
    assert np.array_equal(h.astype(np.float64), gf.layer_input64(sp, x))   # the front layer is exact: the layer under test reads float32 numbers
    return case, sp, r, h


def localised_defects(case, h, z):
    """{name: defective pre-activation}: copies of z (n, OH, OW, OC) with one localised defect each"""
    L = case.layers[-1]
    out = {}
    # one 32-deep k-tile of one element: an input pixel reaches an output element through one tap, so its channels 0 .. 31 are one k-tile
    alt = h.astype(np.float64)
    pix = (h.shape[0] // 2, h.shape[1] // 2, h.shape[2] // 2)
    alt[pix + (slice(0, 32),)] = 0.0
    z_alt = family_ref.forward_specs64([dict(gf.specs(case)[-1], act="linear")], alt)
    fed = np.argwhere(z_alt != z)
    assert len(fed) >= 1
    e = tuple(fed[len(fed) // 2])
    d = z.copy()
    d[e] = z_alt[e]
    out["one 32-deep k-tile left out of one element"] = d
    # one 32-channel sub-block from the neighbouring phase (a layer without phases: from the neighbouring sub-block)
    d = z.copy()
    if L["kind"] == "conv2d_transpose":
        s = L["stride"]
        other = z[:, 0::s, 1::s, 0:32]
        here = d[:, 0::s, 0::s, 0:32]
        here[:, :, :other.shape[2]] = other[:, :, :here.shape[2]]
    else:
        d[..., 0:32] = z[..., 32:64]
    out["one 32-channel sub-block taken from the neighbouring phase"] = d
    # one output row from the next pixel
    d = z.copy().reshape(-1, z.shape[-1])
    row = d.shape[0] // 3
    d[row] = z.reshape(-1, z.shape[-1])[row + 1]
    out["one output row taken from the next pixel"] = d.reshape(z.shape)
    return out


def emulate32(sp, h, prods32):
    """float32 emulation of the kernels' arithmetic: hi x hi in one accumulator, the five small products in a second one in the order
    they are issued, the two met in one add, then the bias"""
    acc_r = np.zeros_like(prods32["h", "h"])
    for key in xf.SMALL:
        acc_r = acc_r + prods32[key]
    z = (prods32["h", "h"] + acc_r) + np.asarray(sp[-1]["b"], np.float32)
    assert z.dtype == np.float32
    return z


@pytest.mark.parametrize("name", [c.name for c in xf.CASES])
def test_the_statistic_rejects_defects_and_accepts_the_kernels_arithmetic(oracle, name):
    case, sp, r, h = numbers(name)
    act = case.layers[-1]["act"]
    limit = gf.bound(r.q_cpu, act)   # without the activation term: the strictest form of the rule
    b = np.asarray(sp[-1]["b"], np.float64)
    z = family_ref.forward_specs64([dict(sp[-1], act="linear")], h.astype(np.float64))
    assert gf.statistic(oracle._act(z, act), r.T, r.S) == 0.0
    # the six products summed in float64: what the scheme itself gives up (the three terms below 2^-24 of a product)
    p64 = xf.products(sp, h)
    six = sum(p64.values()) + b
    q6 = gf.statistic(oracle._act(six, act), r.T, r.S)
    print(f"{name}: q_cpu {r.q_cpu:.3e}, bound {limit:.3e}, six products in float64 q {q6:.3e}")
    assert q6 < gf.TINY, "the scheme would need a floor of its own"
    # accepted: the kernels' arithmetic in float32
    z32 = emulate32(sp, h, xf.products(sp, h, np.float32))
    y32 = oracle._act(z32.astype(np.float64), act).astype(np.float32)
    q32 = gf.statistic(y32, r.T, r.S)
    print(f"  float32 emulation of the two accumulator sets: q {q32:.3e} = {q32 / limit * gf.MARGIN:.2f} of max(q_cpu, floor)")
    assert q32 <= limit and gf.accepts(r.cpu32, r, act)
    # rejected: one of the five small products left out of the whole layer
    if act == "linear":
        assert name in xf.LINEAR_CASES
        for key in xf.SMALL:
            y = six - p64[key]
            q = gf.statistic(y, r.T, r.S)
            print(f"  without weights' {key[0]} x activations' {key[1]}: q {q:.3e} = {q / limit:.1f} x the bound")
            assert q > limit and not gf.accepts(y, r, act), key
    # rejected: the localised defects
    bad = localised_defects(case, h, z)
    assert len(bad) == 3
    for what, zd in bad.items():
        y = oracle._act(zd, act)
        q = gf.statistic(y, r.T, r.S)
        hit = int((gf.q_map(y, r.T, r.S) > limit).sum())
        print(f"  {what}: q {q:.3e} = {q / limit:.1f} x the bound, {hit} element(s) over it")
        assert q > limit and not gf.accepts(y, r, act), what
        if "one element" in what:
            assert hit == 1   # a defect confined to one element is caught in that element alone


def test_the_split_is_exact():
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.standard_normal(4096), [0.0, -0.0, 1.0, 2.0 ** -126, -(2.0 ** 127), 3.4e38]]).astype(np.float32)
    hi, mid, lo = xf.split3(a)
    assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64), a.astype(np.float64))
    for part in (hi, mid, lo):   # each term is a bfloat16: what the packs keep is all of it
        assert not (part.view(np.uint32) & np.uint32(0xffff)).any()
