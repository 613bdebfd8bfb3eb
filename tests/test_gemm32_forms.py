"""The table of f32 GEMM launch forms (tests/gemm32_forms.py) on a CPU: that every case reaches the form it is in the table for and
that the table reaches every form, proved from the library's own plan of the table's graphs -- tools/pack_digest.cpp --forms, the
sanitizer-built harness, dumps plan_gemm32's answer for every layer at the case's batch, and srcfd_model_f32_steps says which
kernel the engine's launch loop would send each layer to under the case's switches -- and that the per-element statistic of
tests/test_gpu_gemm32_forms.py rejects a defect confined to one element, one column block, one phase or one slab while it accepts
a second float32 evaluation that sums in another order.  A case that stops reaching its form fails here, without a GPU."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import family_ref
import gemm32_forms as gf
import gemm32_plan_ref as ref
from conftest import ROOT
from test_gemm32_plan import read_plan_lines


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


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{case name: launches (test_gemm32_plan.read_plan's dicts + layer, big)} of one sanitizer-clean run of the harness"""
    tmp = tmp_path_factory.mktemp("gemm32_forms")
    (tmp / "forms.txt").write_text(gf.forms_text())
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sr-for-cfd_amd", "csrc"), "pack_digest"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "sr-for-cfd_amd", "lib", "pack_digest_asan"), "--forms", str(tmp / "forms.txt"), str(tmp)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]   # ASan / UBSan clean
    cases, lines, extra = {}, None, None
    for line in open(tmp / "forms.gemm32.plan.txt"):
        w = line.split()
        if w[0] == "C":
            lines, extra = [], []
            cases[w[1]] = (int(w[2]), lines, extra)
        elif w[0] == "B":
            extra.append([int(v) for v in w[1:]])
        else:
            lines.append(line)
    got = {}
    for name, (n, lines, extra) in cases.items():
        launches = read_plan_lines(lines)
        assert len(launches) == len(extra) and all(g["n"] == n and g["mode"] == 0 for g in launches), name
        for g, (first, count, layer, big) in zip(launches, extra):
            assert (g["first"], g["count"]) == (first, count), name
            g.update(layer=layer, big=bool(big))
        got[name] = launches
    return got


@pytest.fixture(scope="module")
def steps(srcfd):
    """{case name: (kernel, ops) of the layer under test}: the engine's own choice on a host-only handle, under the case's switches"""
    got = {}
    for c in gf.CASES:
        m = srcfd.SRModel.from_layers(gf.specs(c), c.in_shape, device=-1)
        try:
            with environment(c.env):
                st = m.f32_steps(c.batch)
        finally:
            m.close()
        assert all(k not in ("enc32", "tail32", "triple", "pair", "x3") for _, k, _ in st), (c.name, st)   # nothing fused swallows a layer
        mine = [(k, cnt) for name, k, cnt in st if name.split(".ph")[0] == "under_test"]
        assert len(mine) == 1, (c.name, st)
        got[c.name] = mine[0]
    return got


def test_the_dump_holds_the_table(plans):
    assert list(plans) == [c.name for c in gf.CASES]
    for c in gf.CASES:
        under = [g for g in plans[c.name] if g["layer"] == len(c.layers) - 1]
        assert len(under) == 1 and under[0] is plans[c.name][-1], c.name   # one launch plan: the phases of the layer under test go out together


def test_every_line_matches_the_reference(plans):
    """As tests/test_gemm32_plan.py holds its graphs to tests/gemm32_plan_ref.py: grouped or not, the group's launch, every op's route,
    cut, slab offset, finish groups and own launch, and the slab floats."""
    for name, launches in plans.items():
        for g in launches:
            ds = [o["d"] for o in g["ops"]]
            why, launch, ops = ref.group(ds, True)
            where = (name, g["first"])
            assert g["grouped"] == (why is None), (where, why)
            assert g["launch"] == (launch or dict(nb=0, bkt=0, vec=0, grid=(0, 0, 0), fin=(0, 0))), where
            assert g["ws"] == sum(o["ws"] for o in ops), where
            for got, want in zip(g["ops"], ops):
                ws = want.pop("ws")
                assert got["plan"] == want, (where, got["plan"], want)
                assert got["splitk_ws"] == ws


def split_tags(d, p, tags):
    """of one generic GEMM that is cut"""
    pix = d["MH"] * d["MW"]
    if p["kchunk"] == 144 and d["K"] % 144:
        tags.add("split144:short")
    if p["kchunk"] == 256 and pix == 1 and d["K"] % 256:
        tags.add("split256dense:short")
    if p["kchunk"] == 256 and pix > 1:
        tags.add("split256map")


def classify(case, g, step):
    """The tags a case reaches, from the library's plan `g` of the layer under test and the engine's step for it."""
    L = case.layers[-1]
    kernel, count = step
    ds, ps = [o["d"] for o in g["ops"]], [o["plan"] for o in g["ops"]]
    assert count == g["count"]
    tags = {f"step:{kernel}:{count}" if kernel == "big" else f"step:{kernel}"}
    if any(d["M"] % 128 for d in ds):
        tags.add("M%128")
    if kernel == "big":   # sums the slabs of the batch-invariant cut in registers
        assert g["big"] and not case.env
        if any(p["splits"] > 1 and d["K"] % p["kchunk"] for d, p in zip(ds, ps)):
            tags.add("big:short_slab")
        return tags
    if kernel == "skinny":
        assert not case.env
        if ds[0]["K"] % 4:
            tags.add("skinny:short_k")
        return tags
    if kernel == "finalize":
        assert ps[0]["route"] == "tiled_n1"
        return tags | {f"tiled_n1:{ds[0]['OH']}x{ds[0]['OW']}", f"act:tiled_n1:{L['act']}"}
    assert kernel == ("group" if count > 1 else "mfma") and (not g["big"] or case.env.get("SRCFD_NO_GEMM32_BIG") == "1")
    if count == 1:
        d, p = ds[0], ps[0]
        r = p["route"]
        if (L["kh"], L["kw"], L["cin"], d["M"]) == (1, 1, d["N"], len(gf.probe_z())):
            tags.add("probe:" + r)
        if r == "n1":
            tags |= {"n1", f"act:n1:{L['act']}"} | ({"n1:K=512"} if d["K"] == 512 else set())
        elif r == "n1x4":
            tags |= {"n1x4", f"act:n1x4:{L['act']}"}
        elif r == "ci1":
            tags |= {f"ci1:N={d['N']}:{'same' if L['same'] else 'valid'}", f"act:ci1:{L['act']}"}
        else:
            assert r == "mfma"
            tags.add(f"single:nb{p['nb']}:bkt{p['bkt']}:vec{p['vec']}")
            tags |= {t for t, on in (("M<128", d["M"] < 128), ("M=129", d["M"] == 129), (f"N={d['N']}", d["N"] in gf.EDGE_N), ("K%bkt", d["K"] % p["bkt"] != 0),
                                     ("K<16", d["K"] < 16), ("ci%4,K>32", d["CI"] % 4 != 0 and d["K"] > 32), (f"nphx{d['nphx']}", d["nphx"] > 1),
                                     ("N=1,K>512", d["N"] == 1 and d["K"] > 512), ("n1:K=513", d["N"] == 1 and d["K"] == 513)) if on}
            if L["kind"] == "conv2d" and L["stride"] == 2 and L["same"] and d["ay"] == 2:
                tags |= {"s2same:odd" if side % 2 else "s2same:even" for side in (d["IH"], d["IW"])}
            if p["splits"] > 1:
                split_tags(d, p, tags)
                tags.add("finish8" if p["finish_groups"] == 8 else ("finish1:32slabs" if p["splits"] >= 32 else "finish1"))
                if d["M"] * d["N"] % (256 // p["finish_groups"]):
                    tags.add(f"fin_partial:{p['finish_groups']}")
                tags.add(f"act:finish:{L['act']}")
            else:
                tags.add(f"act:mfma:{L['act']}")
                if L["act"] in gf.NONLINEAR_LOOP:
                    tags.add(f"loop:nb{p['nb']}")
        return tags
    assert L["kind"] == "conv2d_transpose"
    if not g["grouped"]:
        tags.add("nogroup:" + ref.group(ds, True)[0])
        tags |= {t for t, on in (("finish8", any(p["finish_groups"] == 8 for p in ps)), ("convt:n1", any(p["route"] == "n1" for p in ps)),
                                 ("N=1,K>512", any(p["route"] == "mfma" and d["N"] == 1 and d["K"] > 512 for d, p in zip(ds, ps)))) if on}
        return tags
    l = g["launch"]
    tags |= {f"group:nb{l['nb']}:bkt{l['bkt']}:vec{l['vec']}", f"group:count{count}"}
    if (L["kh"], L["kw"], L["stride"]) == (3, 3, 2):
        tags.add("group:same3x3s2" if L["same"] else "group:convt3x3s2")
    if (L["kh"], L["kw"], L["stride"], L["same"]) == (4, 4, 2, False):
        tags.add("group:convt4x4s2")
    if any(ref.ceil_div(d["M"], ref.BM) < l["grid"][0] for d in ds):   # blockIdx.x * BM >= d.M returns early in that phase
        tags.add("group:rows_differ")
    cut = [p["splits"] > 1 for p in ps]
    tags.add("group:allsplit" if all(cut) else ("group:mixed" if any(cut) else "group:nosplit"))
    if any(cut):
        tags.add(f"act:groupfinish:{L['act']}")
        assert l["fin"][0]
        if any(d["M"] * d["N"] % 256 for d, c in zip(ds, cut) if c):
            tags.add("fin_partial:group")
    for d, p in zip(ds, ps):
        if p["splits"] > 1:
            split_tags(d, p, tags)
    return tags


def test_each_case_reaches_the_form_it_names_and_the_table_reaches_every_form(plans, steps):
    reached = set()
    for c in gf.CASES:
        got = classify(c, plans[c.name][-1], steps[c.name])
        assert set(c.reaches) <= got, (c.name, sorted(set(c.reaches) - got), sorted(got))
        reached |= set(c.reaches)
    assert not gf.WANT - reached, sorted(gf.WANT - reached)


def test_the_same_padded_convt_is_the_cropped_one(plans):
    """`group:same3x3s2` means the family's layer: (k - s) // 2 = 0, so the crop takes the VALID result's last row and column, and the
    phases that would hold them, (0, *) and (*, 0) with IH + 1 rows or IW + 1 columns when VALID, run on the input's own grid."""
    for name in ("group4_same3x3", "group4_same3x3_behind_front"):
        ds = [o["d"] for o in plans[name][-1]["ops"]]
        assert {(d["oy0"], d["ox0"]) for d in ds} == {(0, 0), (0, 1), (1, 0), (1, 1)}, name
        assert all((d["MH"], d["MW"], d["OH"], d["OW"]) == (d["IH"], d["IW"], 2 * d["IH"], 2 * d["IW"]) for d in ds), (name, ds)
    valid = [o["d"] for o in plans["group4_3x3"][-1]["ops"]]
    assert {(d["MH"] - d["IH"], d["MW"] - d["IW"]) for d in valid} == {(1, 1), (1, 0), (0, 1), (0, 0)}


def test_the_table_stays_small(plans):
    """Nothing above the NB 4 / BKT 16 cases' 17 M output floats, one forward per call (the ping-pong buffers hold the whole batch)."""
    for c in gf.CASES:
        d = plans[c.name][-1]["ops"][0]["d"]
        out = c.batch * d["OH"] * d["OW"] * d["OC"]
        assert out <= 17.5e6 and c.batch <= 1024, (c.name, out)
        per_sample = max([int(np.prod(c.in_shape))] + [o["d"]["OH"] * o["d"]["OW"] * o["d"]["OC"] for g in plans[c.name] for o in g["ops"]])
        assert 2 * 4 * per_sample * c.batch <= 3 << 30, c.name   # Model::chunk_cap: the call is not cut into chunks


# ---------------------------------------------------------------------------------------------------------------------------------
# the statistic
# ---------------------------------------------------------------------------------------------------------------------------------
STAT_CASES = ("finish1_32_slabs", "group_mixed", "tiled_n1_17x65")   # the largest K, a grouped case, a tiled_n1 case


def pre_activation(sp, h):
    return family_ref.forward_specs64([dict(sp[-1], act="linear")], h)


def defects(case, sp, h, z):
    """{name: defective pre-activation}: copies of z with one localised defect each"""
    L, w, b = case.layers[-1], np.asarray(sp[-1]["w"], np.float64), np.asarray(sp[-1]["b"], np.float64)
    out = {}
    d = z.copy()
    if L["kind"] == "dense":       # z (n, 1, 1, N), h (n, 1, 1, K)
        terms = np.abs(h[7, 0, 0, :] * w[:, 5])
        k = int(np.argsort(terms)[len(terms) // 2])      # a term of median size
        d[7, 0, 0, 5] -= h[7, 0, 0, k] * w[k, 5]
        out["one dropped k-term in one element"] = d
        d = z.copy()
        d[128:256, 0, 0, 32:64] = z[0:128, 0, 0, 32:64]
        out["one 32-column block shifted by one row tile"] = d
        d = z.copy()
        d[:128, 0, 0, :] -= h[:128, 0, 0, 256:512] @ w[256:512]
        out["one slab of one row tile not added"] = d
    elif L["kind"] == "conv2d":    # 3x3 SAME, stride 1: z[img, y, x] sums h[img, y + ty - 1, x + tx - 1, ci] w[ty, tx, ci]
        terms = np.abs(h[1, 8:11, 30:33, :] * w[:, :, :, 0])
        ty, tx, ci = np.unravel_index(int(np.argsort(terms, axis=None)[terms.size // 2]), terms.shape)
        d[1, 9, 31, 0] -= h[1, 8 + ty, 30 + tx, ci] * w[ty, tx, ci, 0]
        out["one dropped k-term in one element"] = d
    else:                          # ConvT 3x3 stride 2 VALID: z[img, 2 i + a, 2 j + b, co] += h[img, i, j, ci] w[a, b, co, ci]
        terms = np.abs(h[1, 2, 3, :] * w[2, 0, 4, :])
        ci = int(np.argsort(terms)[len(terms) // 2])
        d[1, 2 * 2 + 2, 2 * 3 + 0, 4] -= h[1, 2, 3, ci] * w[2, 0, 4, ci]
        out["one dropped k-term in one element"] = d
        d = z.copy()
        d[:, 1::2, 1::2, :] = b
        out["one phase left at bias only"] = d
        d = z.copy()                # phase (0, 0), k = (ty, tx, ci): its first 144-deep slab is tap (0, 0), channels 0 .. 143
        H, W = h.shape[1:3]
        d[:, 0:2 * H:2, 0:2 * W:2, :] -= h[..., :144] @ w[0, 0, :, :144].T
        out["one slab of one phase not added"] = d
    return out


@pytest.mark.parametrize("name", STAT_CASES)
def test_the_statistic_rejects_localised_defects_and_accepts_float32(oracle, plans, name):
    case = gf.BY_NAME[name]
    assert name != STAT_CASES[0] or max(o["d"]["K"] for launches in plans.values() for o in launches[-1]["ops"]) == plans[name][-1]["ops"][0]["d"]["K"]   # the largest K
    sp, x = gf.specs(case), gf.inputs(case)
    r = gf.reference(case, sp, x)
    act = case.layers[-1]["act"]
    limit = gf.bound(r.q_cpu, act)   # without the activation term: the strictest form of the rule
    print(f"{name}: q_cpu {r.q_cpu:.3e}, bound {limit:.3e}")
    np32 = family_ref.forward_specs64(sp, x, np.float32)   # tap-by-tap numpy float32: another order than torch's
    q32 = gf.statistic(np32, r.T, r.S)
    print(f"  numpy float32 evaluation: q {q32:.3e} ({q32 / limit * gf.MARGIN:.2f} of the floor)")
    assert q32 <= limit and gf.accepts(r.cpu32, r, act)
    h = gf.layer_input64(sp, x)
    z = pre_activation(sp, h)
    assert gf.statistic(oracle._act(z, act), r.T, r.S) == 0.0
    bad = defects(case, sp, h, z)
    assert len(bad) == {"finish1_32_slabs": 3, "group_mixed": 3, "tiled_n1_17x65": 1}[name]
    for what, zd in bad.items():
        y = oracle._act(zd, act)
        q = gf.statistic(y, r.T, r.S)
        hit = int((gf.q_map(y, r.T, r.S) > limit).sum())
        print(f"  {what}: q {q:.3e} = {q / limit:.1f} x the bound, {hit} element(s) over it")
        assert q > limit and not gf.accepts(y, r, act), what
        if "one element" in what:
            assert hit == 1   # a defect confined to one element is caught in that element alone


def test_the_statistic_counts_a_nan_and_a_zero_sum():
    T, S = np.array([1.0, 0.0, 2.0]), np.array([1.0, 0.0, 2.0])
    assert gf.statistic(np.array([1.0, 0.0, 2.0]), T, S) == 0.0
    assert gf.statistic(np.array([1.0, 1e-30, 2.0]), T, S) == np.inf     # nothing was summed there: the element has to be met exactly
    assert gf.statistic(np.array([np.nan, 0.0, 2.0]), T, S) == np.inf
    assert gf.bound(0.0) == gf.MARGIN * gf.TINY and gf.bound(1e-6, "swish", 1e-7) == gf.MARGIN * 1e-6 and gf.bound(0.0, "swish", 1e-7) == gf.MARGIN * (gf.TINY + 1e-7)
