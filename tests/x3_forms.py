"""The launch forms of the split-bf16 GEMM (csrc/kernels_x3.hip, precision fp32x3) as a table of small layer graphs, in the style of
tests/gemm32_forms.py, whose Case, specs, inputs, reference and statistic it uses: an optional exact front layer plus the layer under
test, which is the last one.  Every case names the tags (`reaches`) it is in the table for; tests/test_x3_forms.py proves on a CPU,
from the library's own plan of these graphs (csrc/x3_plan.cpp through tools/pack_digest.cpp --forms, `forms.x3.plan.txt`) and from
the engine's own step list at fp32x3, that each case reaches its tags and that the tags of WANT are all reached;
tests/test_gpu_x3_forms.py runs every case on the device against float64, per element.

Every batch is >= 64: the precision uses these kernels from 64 samples per call on.  Spatial sizes are a few pixels; the one large
case (res_second_tile, 66 495 rows) is the smallest at which a wave of the weights-resident kernel takes a second tile on 256 CUs.
CO: output channels per phase; a 128-channel column block is `by` of `nby`, a resident kernel's channel block one of `nblk`.

The statistic and its bound are gemm32_forms': max_i q_i <= 8 x max(q_cpu, 2^-24 [+ the activation's own error]).  The six-product
scheme needs no floor of its own: summed in float64 its q is 0.5 to 5e-8 (tests/test_x3_forms.py prints it per case), below 2^-24,
while one small product left out costs 1e-6 and more."""
import os
import subprocess

import numpy as np

import gemm32_forms as gf
import x3_plan_ref as ref
from gemm32_forms import Case, FLATTEN, conv, convt, dense, front

PROBE_W, PROBE_N = 63, 64   # the activation probe: probe_z() laid out over 64 samples x 63 pixels (zeros behind the last one)
KERNELS = ("tile", "group", "res")


def _table():
    t = []

    def add(name, in_shape, batch, layers, reaches):
        assert batch >= 64
        t.append(Case(name, tuple(in_shape), batch, tuple(layers), tuple(reaches), {}))

    # ---- gemm_x3, one launch ---------------------------------------------------------------------------------------------------------
    add("tile_same3x3", (9, 7, 64), 64, [conv(64, 128, 3, same=True, act="swish")],
        ["tile:single", "check:all_sides", "tile:wave_past_M", "M%128", "act:tile:swish"])   # K = 576; M = 4032 = 31 x 128 + 64
    add("tile_valid3x3", (8, 8, 32), 65, [conv(32, 128, 3)], ["tile:single", "tile:kt_odd", "tile:tap_per_ktile", "M%32", "act:tile:linear"])   # K = 288
    add("tile_s2same_even", (10, 10, 32), 64, [conv(32, 128, 3, stride=2, same=True, act="swish")], ["tile:single", "s2same:even"])
    add("tile_s2same_odd", (9, 9, 32), 64, [conv(32, 128, 3, stride=2, same=True, act="swish")], ["tile:single", "s2same:odd"])
    add("tile_k128", (5, 6, 32), 64, [conv(32, 128, 2, act="swish")], ["tile:single", "tile:K=128"])
    add("tile_1x1", (5, 5, 256), 67, [conv(256, 256, 1, act="swish")], ["tile:single", "tile:nocheck_rows_past_M", "tile:nby2", "M%32"])
    add("tile_dense", (2, 2, 3), 65, [front(3, 64), FLATTEN, dense(256, 128, act="swish")], ["tile:single", "dense", "M<128", "M%32"])
    add("tile_convt_sub32", (6, 6, 256), 64, [convt(256, 32, 2, 2, act="swish")], ["tile:single", "tile:phase:sub32"])
    add("tile_convt_span96", (6, 6, 256), 64, [convt(256, 96, 2, 2)], ["tile:single", "tile:phase:span", "tile:nby2", "act:tile:linear"])
    add("tile_convt_k3s3", (4, 5, 256), 64, [convt(256, 128, 3, 3, act="swish")], ["tile:single", "tile:phase:merged9"])
    # ---- gemm_x3_group ---------------------------------------------------------------------------------------------------------------
    add("group4_3x3", (5, 6, 256), 64, [convt(256, 128, 3, 2, act="swish")], ["group:count4", "group:convt3x3s2", "group:rows_differ", "act:group:swish"])
    add("group4_same3x3", (5, 5, 256), 64, [convt(256, 128, 3, 2, same=True, act="swish")], ["group:count4", "group:same3x3s2"])
    add("group4_4x4", (5, 5, 64), 64, [convt(64, 128, 4, 2)], ["group:count4", "group:convt4x4s2", "act:group:linear"])
    add("group2", (1, 9, 256), 64, [convt(256, 128, 1, 2, kw=3, act="swish")], ["group:count2"])
    add("group3", (1, 7, 256), 64, [convt(256, 128, 1, 3, kw=4)], ["group:count3", "act:group:linear"])
    add("group4_nby2", (4, 4, 256), 64, [convt(256, 256, 3, 2, act="swish")], ["group:count4", "group:nby2", "group:rows_differ"])
    # ---- not grouped: the one-tap phase of a 128-channel 3x3 stride-2 ConvT goes to the resident kernel ------------------------------
    add("nogroup_res_member", (5, 6, 128), 64, [convt(128, 128, 3, 2, act="swish")], ["nogroup:member", "nogroup:tile3+res1"])
    # ---- gemm_x3_res -----------------------------------------------------------------------------------------------------------------
    add("res_convt_k2", (7, 5, 128), 70, [convt(128, 64, 2, 2, act="swish")], ["res", "res:nblk2", "res:one_tile_per_wave", "res:last_tile_partial", "act:res:swish"])
    add("res_1x1", (6, 7, 128), 64, [conv(128, 128, 1)], ["res", "act:res:linear"])
    add("res_convt_k3s3", (4, 5, 128), 64, [convt(128, 128, 3, 3, act="swish")], ["res", "res:nblk9", "res:phase:merged9"])
    add("res_second_tile", (31, 33, 128), 65, [convt(128, 32, 2, 2)],
        ["res", "res:second_tile", "res:last_tile_partial", "res:phase:sub32", "act:res:linear"])   # M = 66 495: 2078 tiles on 2048 wave slots
    # ---- the graphs of the activation probe (test_gpu_x3_forms.py: identity weights, zero bias), here with ordinary numbers ----------
    add("probe_res", (1, PROBE_W, 128), PROBE_N, [conv(128, 128, 1, act="swish")], ["res", "probe:res"])
    add("probe_tile", (1, PROBE_W, 256), PROBE_N, [conv(256, 256, 1, act="swish")], ["tile:single", "probe:tile"])
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
LINEAR_CASES = tuple(c.name for c in CASES if c.layers[-1]["act"] == "linear")

# what the table must reach between its cases: the three kernels; a group of 2, 3 and 4 ops and a layer that is not grouped because
# the resident kernel takes a member; the M, N, K and phase forms of each kernel; swish and linear on each kernel; the probe's graphs
WANT = {"tile:single", "res", "group:count2", "group:count3", "group:count4", "nogroup:member", "nogroup:tile3+res1"}
WANT |= {"M<128", "M%32", "M%128", "tile:wave_past_M", "tile:nocheck_rows_past_M", "group:rows_differ", "res:one_tile_per_wave", "res:second_tile",
         "res:last_tile_partial"}
WANT |= {"tile:nby2", "group:nby2", "res:nblk2", "res:nblk9"}
WANT |= {"tile:K=128", "tile:kt_odd", "tile:tap_per_ktile", "dense"}
WANT |= {"tile:phase:sub32", "tile:phase:span", "tile:phase:merged9", "res:phase:sub32", "res:phase:merged9"}
WANT |= {"check:all_sides", "s2same:odd", "s2same:even", "group:convt3x3s2", "group:same3x3s2", "group:convt4x4s2"}
WANT |= {f"act:{k}:{a}" for k in KERNELS for a in ("swish", "linear")} | {"probe:res", "probe:tile"}

FIELDS = ref.FIELDS


def layer_descriptors(case):
    """the GEMM descriptors of the layer under test as tests/x3_plan_ref.py derives them (no dump: the device test's source)"""
    h, w, c = case.in_shape
    for l in case.layers[:-1]:
        if l["kind"] == "flatten":
            h, w, c = 1, 1, h * w * c
        else:
            assert l["kind"] == "conv2d" and (l["kh"], l["kw"], l["stride"]) == (1, 1, 1) and l["cin"] == c   # a front layer keeps the grid
            c = l["cout"]
    assert case.layers[-1]["cin"] == c
    return ref.descriptors(case.layers[-1], h, w, case.batch)


def dump_plans(tmp, root):
    """{case name: [layer plans]} of one run of the sanitizer-built harness over the table, written below `tmp`; a layer plan is
    dict(first, count, layer, cus, grouped, group_grid, first5, ops=[dict(kernel, kpad, grid, ntiles, res, d)]): one per layer that
    gemm_x3_qualifies accepts whole."""
    forms = os.path.join(str(tmp), "forms.txt")
    with open(forms, "w") as f:
        f.write(gf.forms_text(CASES))
    subprocess.check_call(["make", "-C", os.path.join(root, "sr-for-cfd_amd", "csrc"), "pack_digest"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(root, "sr-for-cfd_amd", "lib", "pack_digest_asan"), "--forms", forms, str(tmp)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]   # ASan / UBSan clean
    got, layers = {}, None
    for line in open(os.path.join(str(tmp), "forms.x3.plan.txt")):
        kind, *w = line.split()
        if kind == "C":
            layers = got.setdefault(w[0], [])
            batch = int(w[1])
            continue
        v = [int(x) for x in w]
        if kind == "X":
            layers.append(dict(first=v[0], count=v[1], layer=v[2], cus=v[3], grouped=bool(v[4]), group_grid=v[5], first5=tuple(v[6:11]), ops=[], n=batch))
        else:
            assert kind == "P" and len(v) == 7 + len(FIELDS)
            g = layers[-1]
            assert v[0] == g["first"] + len(g["ops"]) and len(g["ops"]) < g["count"]
            g["ops"].append(dict(kernel=ref.KERNELS[v[1]], kpad=v[2], grid=(v[3], v[4]), ntiles=v[5], res=bool(v[6]), d=dict(zip(FIELDS, v[7:]))))
    assert all(len(g["ops"]) == g["count"] for ls in got.values() for g in ls)
    return got


def reference_plan(ds, num_cus):
    """the layer plan (as dump_plans') that tests/x3_plan_ref.py gives for these descriptors on `num_cus` CUs"""
    why, launch, ops = ref.group(ds, num_cus)
    return dict(count=len(ds), cus=num_cus, grouped=why is None, group_grid=launch[0] if launch else 0, first5=launch[1] if launch else (0,) * 5,
                ops=[dict(o, res=ref.res_qualifies(d), d=d) for o, d in zip(ops, ds)])


def classify(case, g):
    """The tags a case reaches, from a plan `g` (the library's or the reference's) of the layer under test."""
    L = case.layers[-1]
    ds, ops = [o["d"] for o in g["ops"]], g["ops"]
    act = L["act"]
    tags = set()
    if g["count"] > 1:
        assert L["kind"] == "conv2d_transpose"
        if not g["grouped"]:
            tags.add("nogroup:" + ref.group(ds, g["cus"])[0])
            kinds = [o["kernel"] for o in ops]
            tags.add(f"nogroup:tile{kinds.count('tile')}+res{kinds.count('res')}")
            return tags
        assert all(o["kernel"] == "tile" for o in ops)
        tags |= {f"group:count{g['count']}", f"act:group:{act}"}
        if (L["kh"], L["kw"], L["stride"]) == (3, 3, 2):
            tags.add("group:same3x3s2" if L["same"] else "group:convt3x3s2")
        if (L["kh"], L["kw"], L["stride"], L["same"]) == (4, 4, 2, False):
            tags.add("group:convt4x4s2")
        if len({ref.ceil_div(d["M"], ref.BP) for d in ds}) > 1:
            tags.add("group:rows_differ")
        if ds[0]["N"] // ref.BN >= 2:
            tags.add("group:nby2")
        return tags
    d, o = ds[0], ops[0]
    M = d["M"]
    tags |= {t for t, on in (("M<128", M < 128), ("M%32", M % 32 != 0), ("M%128", M % 128 != 0), ("dense", L["kind"] == "dense")) if on}
    if (L["kh"], L["kw"], L["cin"]) == (1, 1, L["cout"]) and case.in_shape[:2] == (1, PROBE_W) and case.batch == PROBE_N:
        tags.add("probe:" + o["kernel"])
    if o["kernel"] == "res":
        slots = 8 * o["grid"][0]
        tags |= {"res", f"act:res:{act}", f"res:nblk{o['grid'][1]}", "res:one_tile_per_wave" if o["ntiles"] <= slots else "res:second_tile"}
        tags |= {t for t, on in (("res:last_tile_partial", M % 32 != 0), ("res:phase:sub32", d["nphx"] > 1 and d["CO"] == 32), ("res:phase:merged9", d["nphx"] == 3)) if on}
        assert o["ntiles"] <= 2 * slots   # a third tile is no other path than the second
        return tags
    check = d["TY"] * d["TX"] > 1 or d["cy"] != 0 or d["cx"] != 0
    tags |= {"tile:single", f"act:tile:{act}"}
    tags |= {t for t, on in (("tile:wave_past_M", 0 < M % 128 <= 96), ("tile:nocheck_rows_past_M", not check and M % 32 != 0), ("tile:nby2", d["N"] // ref.BN >= 2),
                             ("tile:K=128", d["K"] == 128), ("tile:kt_odd", o["kpad"] // ref.BK % 2 == 1), ("tile:tap_per_ktile", d["CI"] == ref.BK and d["TY"] * d["TX"] > 1),
                             ("tile:phase:sub32", d["nphx"] > 1 and d["CO"] == 32), ("tile:phase:span", d["nphx"] > 1 and d["CO"] % ref.BN != 0 and ref.BN % d["CO"] != 0),
                             ("tile:phase:merged9", d["nphx"] == 3),
                             ("check:all_sides", L["kind"] == "conv2d" and L["same"] and L["stride"] == 1 and d["cy"] < 0 and d["cx"] < 0 and d["TY"] == 3 and d["TX"] == 3)) if on}
    if L["kind"] == "conv2d" and L["stride"] == 2 and L["same"] and d["ay"] == 2:
        tags |= {"s2same:odd" if side % 2 else "s2same:even" for side in (d["IH"], d["IW"])}
    return tags


# ---------------------------------------------------------------------------------------------------------------------------------
# the six-product scheme on a CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def split3(a):
    """float32 -> (hi, mid, lo) float32 with hi + mid + lo == a exactly: the truncation split of kernels_x3.hip (split8) and of the
    host's weight planes (operand_pack.cpp, split3): the low 16 bits cleared, twice"""
    a = np.ascontiguousarray(a, np.float32)
    hi = (a.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    r1 = a - hi
    mid = (r1.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    lo = r1 - mid
    return hi, mid, lo


SMALL = (("m", "m"), ("h", "l"), ("l", "h"), ("h", "m"), ("m", "h"))   # (weight plane, activation plane) in the order the kernels issue them


def products(sp, h, dtype=np.float64):
    """{(weight plane, activation plane): the layer under test without bias and activation on those planes}, summed in `dtype`; h: the
    layer's float32 input"""
    import family_ref
    xs = dict(zip("hml", split3(h)))
    ws = dict(zip("hml", split3(np.asarray(sp[-1]["w"], np.float32))))
    zero = np.zeros_like(np.asarray(sp[-1]["b"], dtype))
    return {(p, q): family_ref.forward_specs64([dict(sp[-1], w=ws[p].astype(dtype), b=zero, act="linear")], xs[q].astype(dtype), dtype)
            for p, q in (("h", "h"),) + SMALL}
