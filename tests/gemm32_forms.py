"""The launch forms of the f32 GEMM as a table of small layer graphs for `SRModel.from_layers`, each with a batch size: an optional
cheap front layer plus the layer under test, which is the last one, so that its output is what a test reads.  Every case names the
tags (`reaches`) it is in the table for; tests/test_gemm32_forms.py proves on a CPU, from the library's own plan of these graphs
(tools/pack_digest.cpp --forms) and from the engine's own step list (srcfd_model_f32_steps), that each case reaches its tags and
that the tags of WANT are all reached; tests/test_gpu_gemm32_forms.py runs every case on the device against float64, per element.

The statistic.  For output element i of the layer under test, T_i is its float64 value and S_i = sum_k |x_k w_k| + |b| the same sum
over absolute values (float64, one more product); q_i = |y_i - T_i| / (S_i + |T_i|).  A case passes when
max_i q_i <= MARGIN * max(q_cpu, floor), q_cpu the same maximum for a float32 CPU evaluation of the same graph (torch).  MARGIN = 8
is the project's rule for two float32 evaluations of one sum in different orders (RATIO, tests/test_gpu_training_oracle.py); the
floor is 2^-24, the half-ulp that any one rounding of a result of size S + |T| may cost, plus, under a nonlinear activation, the
error of the device's activation measured on an exact GEMM (test_gpu_gemm32_forms.py, activation_error).

A front layer is exact: its inputs are multiples of 1/16 in [-2, 2], its weights and biases multiples of 1/8 in [-1, 1], K <= 16 and
its activation linear or relu, so every partial sum is a multiple of 2^-7 below 2^6 and float32 adds it without rounding in any
order.  The layer under test therefore reads the same numbers on the device, in torch and in float64.

Shapes are the smallest that reach a form.  (row tiles x slabs x column blocks) >= 1024 turns the K tile to 16 deep and >= 512 keeps
the widest column blocking, so the NB 4 / BKT 16 cases need 1024 row tiles: 131 000 rows of 97 .. 128 channels, 13 - 17 M output
floats with K of 8 or 12; nothing is larger.  Two forms of the plan cannot be reached by a layer graph and are not in the table:
a layer's phases never differ in width (`npad`) or in CI % 4 (`ci4`); the plan test keeps them on hand-altered descriptors."""
import importlib
from collections import namedtuple

import numpy as np

MARGIN = 8.0
TINY = 2.0 ** -24
ACTS = ("linear", "swish", "relu", "tanh", "sigmoid")
NONLINEAR_LOOP = ("relu", "tanh", "sigmoid")   # the mfma epilogue's register-select loop
EDGE_N = (31, 33, 65, 127, 129)

Case = namedtuple("Case", "name in_shape batch layers reaches env")


def conv(cin, cout, k, stride=1, same=False, act="linear", exact=False):
    return dict(kind="conv2d", kh=k, kw=k, stride=stride, same=same, cin=cin, cout=cout, act=act, exact=exact)


def convt(cin, cout, kh, stride, same=False, act="linear", kw=None):
    return dict(kind="conv2d_transpose", kh=kh, kw=kw or kh, stride=stride, same=same, cin=cin, cout=cout, act=act, exact=False)


def dense(cin, cout, act="linear"):
    return dict(kind="dense", kh=1, kw=1, stride=1, same=False, cin=cin, cout=cout, act=act, exact=False)


FLATTEN = dict(kind="flatten", kh=1, kw=1, stride=1, same=False, cin=0, cout=0, act="linear", exact=False)


def front(cin, cout, act="relu"):
    """the exact front layer: a 1x1 convolution"""
    return conv(cin, cout, 1, act=act, exact=True)


def probe_z():
    """pre-activations of the activation probe: [-100, 100] in steps of 0.05, the edges of float32's exp range, zeros, denormals, infinities"""
    edge = [s * (88.0 + d) for s in (1, -1) for d in (-1, 0, 1)]
    tiny = [s * v for s in (1, -1) for v in (0.0, 2.0 ** -149, 1e-40, 2.0 ** -127, 2.0 ** -126)]
    return np.concatenate([np.linspace(-100, 100, 4001), edge, tiny, [np.inf, -np.inf]]).astype(np.float32)


def _table():
    t = []

    def add(name, in_shape, batch, layers, reaches, env=None):
        t.append(Case(name, tuple(in_shape), batch, tuple(layers), tuple(reaches), dict(env or {})))

    # ---- gemm_mfma_f32, single launch: NB x BKT x VEC, and the edge shapes -------------------------------------------------------
    add("nb1_b32_v0", (7, 9, 5), 2, [conv(5, 31, 3, same=True, act="swish")],
        ["single:nb1:bkt32:vec0", "M<128", "N=31", "K%bkt", "ci%4,K>32", "act:mfma:swish"])
    add("nb1_b32_v1", (5, 45, 4), 1, [conv(4, 33, 3)], ["single:nb1:bkt32:vec1", "M=129", "N=33", "K%bkt", "act:mfma:linear"])
    add("nb1_b16_v0", (38, 60, 3), 20, [conv(3, 65, 2, act="relu")],
        ["single:nb1:bkt16:vec0", "M%128", "N=65", "K<16", "K%bkt", "act:mfma:relu", "loop:nb1"])
    add("nb1_b16_v1", (37, 59, 8), 60, [conv(8, 31, 1, act="tanh")], ["single:nb1:bkt16:vec1", "M%128", "N=31", "K<16", "act:mfma:tanh", "loop:nb1"])
    add("nb2_b32_v0", (38, 60, 3), 31, [conv(3, 33, 2, act="sigmoid")],
        ["single:nb2:bkt32:vec0", "M%128", "N=33", "K<16", "act:mfma:sigmoid", "loop:nb2"])
    add("nb2_b32_v1", (37, 59, 8), 11, [conv(8, 161, 1, act="swish")], ["single:nb2:bkt32:vec1", "M%128", "K<16"])
    add("nb2_b16_v0", (38, 60, 3), 20, [conv(3, 170, 2)], ["single:nb2:bkt16:vec0", "M%128", "K<16"])
    add("nb2_b16_v1", (37, 59, 8), 20, [conv(8, 192, 1, act="relu")], ["single:nb2:bkt16:vec1", "M%128", "loop:nb2"])
    add("nb4_b32_v0", (38, 60, 3), 31, [conv(3, 127, 2, act="tanh")], ["single:nb4:bkt32:vec0", "M%128", "N=127", "loop:nb4"])
    add("nb4_b32_v1", (37, 59, 8), 31, [conv(8, 100, 1)], ["single:nb4:bkt32:vec1", "M%128"])
    add("nb4_b16_v0", (38, 60, 3), 60, [conv(3, 97, 2, act="swish")], ["single:nb4:bkt16:vec0", "M%128"])
    add("nb4_b16_v1", (37, 59, 8), 60, [conv(8, 128, 1)], ["single:nb4:bkt16:vec1", "M%128"])
    add("n129", (6, 11, 8), 3, [conv(8, 129, 3, same=True, act="sigmoid")], ["N=129", "M%128", "K%bkt", "loop:nb1"])   # 160 padded columns: five blocks of 32
    add("s2same_odd", (9, 9, 1), 3, [conv(1, 16, 3, stride=2, same=True, act="swish")], ["s2same:odd", "K<16", "M<128"])
    add("s2same_even", (10, 10, 1), 3, [conv(1, 12, 3, stride=2, same=True, act="swish")], ["s2same:even", "K<16"])
    add("s2same_mixed_behind_front", (9, 10, 2), 3, [front(2, 6), conv(6, 20, 3, stride=2, same=True, act="relu")], ["s2same:odd", "s2same:even", "ci%4,K>32"])
    add("convt_k2s2", (5, 7, 12), 3, [convt(12, 5, 2, 2, act="swish")], ["nphx2", "K<16", "M<128"])
    add("convt_k3s3", (4, 5, 6), 2, [convt(6, 7, 3, 3, act="tanh")], ["nphx3", "K<16", "loop:nb1"])
    # ---- split-K, single launch --------------------------------------------------------------------------------------------------
    for act in ACTS:
        add(f"split144_{act}", (5, 7, 60), 3, [conv(60, 20, 3, same=True, act=act)], ["split144:short", "fin_partial:1", f"act:finish:{act}"])
    add("split256_dense", (2, 2, 3), 5, [front(3, 275), FLATTEN, dense(1100, 50, act="swish")], ["split256dense:short", "fin_partial:1"])
    add("split256_map", (9, 9, 64), 2, [conv(64, 24, 3, same=True, act="swish")], ["split256map", "fin_partial:1"])
    add("finish8", (1, 1, 8200), 3, [dense(8200, 40, act="swish")], ["finish8", "fin_partial:8", "split256dense:short"])
    add("finish1_32_slabs", (1, 1, 8200), 300, [dense(8200, 219, act="swish")], ["finish1:32slabs", "fin_partial:1", "M%128"])
    # ---- gemm_mfma_group_f32 ---------------------------------------------------------------------------------------------------------
    add("group4_3x3", (5, 6, 8), 4, [convt(8, 20, 3, 2, act="swish")],
        ["group:nb1:bkt32:vec1", "group:count4", "group:convt3x3s2", "group:rows_differ", "group:nosplit"])
    add("group4_4x4", (4, 5, 6), 2, [convt(6, 9, 4, 2, act="relu")], ["group:nb1:bkt32:vec0", "group:count4", "group:convt4x4s2", "group:nosplit"])
    add("group4_same3x3", (5, 5, 8), 3, [convt(8, 12, 3, 2, same=True, act="swish")], ["group:count4", "group:same3x3s2", "group:nosplit"])
    add("group4_same3x3_behind_front", (6, 5, 3), 11, [front(3, 16), convt(16, 36, 3, 2, same=True, act="swish")], ["group:count4", "group:same3x3s2", "M%128"])
    add("group2", (1, 9, 8), 3, [convt(8, 10, 1, 2, kw=3, act="swish")], ["group:count2", "group:nosplit"])
    add("group3", (1, 7, 5), 2, [convt(5, 6, 1, 3, kw=4, act="tanh")], ["group:count3", "group:nosplit"])
    for act in ACTS:
        add(f"group_allsplit_{act}", (5, 5, 128), 2, [convt(128, 16, 4, 2, act=act)], ["group:allsplit", "group:count4", "fin_partial:group", f"act:groupfinish:{act}"])
    add("group_mixed", (6, 7, 256), 2, [convt(256, 24, 3, 2, act="swish")], ["group:mixed", "group:count4", "fin_partial:group"])
    add("group_mixed_behind_front", (6, 7, 2), 3, [front(2, 256), convt(256, 40, 3, 2, act="tanh")], ["group:mixed", "group:count4"])
    for nb, bkt, vec, n, cout in ((1, 16, 0, 60, 20), (1, 16, 1, 60, 24), (2, 32, 0, 30, 40), (2, 32, 1, 30, 64), (2, 16, 0, 60, 33), (2, 16, 1, 60, 48),
                                  (4, 32, 0, 30, 97), (4, 32, 1, 30, 128), (4, 16, 0, 60, 97), (4, 16, 1, 60, 100)):
        act = ("swish", "linear", "relu")[(nb + bkt // 16 + vec) % 3]
        add(f"group_nb{nb}_b{bkt}_v{vec}", (20, 27, 4 if vec else 2), n, [convt(4 if vec else 2, cout, 3, 2, act=act)],
            [f"group:nb{nb}:bkt{bkt}:vec{vec}", "group:count4", "group:rows_differ", "group:nosplit"])
    # ---- every way of not being grouped that a layer graph has ---------------------------------------------------------------------
    add("nogroup_finish8", (3, 3, 1160), 2, [convt(1160, 8, 3, 2, act="swish")], ["nogroup:finish8", "finish8"])
    add("nogroup_member_n1", (5, 6, 4), 3, [convt(4, 1, 3, 2, act="swish")], ["nogroup:member", "convt:n1"])
    add("nogroup_member_mixed", (4, 5, 200), 2, [convt(200, 1, 3, 2, act="swish")], ["nogroup:member", "convt:n1", "N=1,K>512"])
    # ---- the conv kernels ----------------------------------------------------------------------------------------------------------
    for (h, w), act in zip(((1, 1), (15, 63), (17, 65), (16, 64), (33, 130)), ACTS):
        add(f"tiled_n1_{h}x{w}", (h, w, 8), 3, [conv(8, 1, 3, same=True, act=act)], [f"tiled_n1:{h}x{w}", f"act:tiled_n1:{act}"])
    add("tiled_n1_behind_front", (17, 65, 2), 2, [front(2, 8), conv(8, 1, 3, same=True, act="swish")], ["tiled_n1:17x65"])
    for act in ACTS:
        add(f"n1x4_{act}", (19, 38, 8), 3, [conv(8, 1, 3, act=act)], ["n1x4", f"act:n1x4:{act}"])
    for act in ACTS:
        add(f"n1_{act}", (6, 7, 3), 3, [conv(3, 1, 3, same=True, act=act)], ["n1", f"act:n1:{act}"])
    add("n1_k512", (4, 5, 128), 70, [conv(128, 1, 2, act="swish")], ["n1", "n1:K=512"])
    add("n1_k513_to_mfma", (4, 5, 57), 3, [conv(57, 1, 3, same=True, act="swish")], ["N=1,K>512", "n1:K=513"])
    add("n1_dense", (1, 1, 300), 7, [dense(300, 1, act="tanh")], ["n1"])
    for n, act in zip(range(1, 9), ("swish",) + ACTS + ("relu", "tanh")):   # one output channel goes to conv_n1_f32 first
        same = n % 2 == 0
        add(f"ci1_n{n}_{'same' if same else 'valid'}", (9, 11, 1), 30, [conv(1, n, 3 if n < 6 else 5, stride=2 if n == 4 else 1, same=same, act=act)],
            (["n1"] if n == 1 else [f"ci1:N={n}:{'same' if same else 'valid'}", f"act:ci1:{act}"]))
    # ---- the graphs of the activation probe (test_gpu_gemm32_forms.py: identity weights, zero bias), here with ordinary numbers ------
    add("probe_mfma", (1, len(probe_z()), 2), 1, [conv(2, 2, 1, act="swish")], ["single:nb1:bkt32:vec0", "K<16", "probe:mfma"])
    add("probe_n1", (1, len(probe_z()), 1), 1, [conv(1, 1, 1, act="swish")], ["n1", "probe:n1"])
    # ---- the two kernels that pre-empt the generic ones, and the same cases with them switched off -----------------------------------
    big1 = ((15, 15, 64), 583, [conv(64, 128, 3, same=True, act="swish")])
    big4 = ((7, 7, 4), 583, [front(4, 128), convt(128, 128, 3, 2, act="swish")])
    skinny = ((1, 1, 50), 130, [dense(50, 9216, act="swish")])
    add("gemm32_big_1", *big1, ["step:big:1", "M%128", "big:short_slab"])
    add("gemm32_big_1_off", *big1, ["step:mfma", "single:nb4:bkt16:vec1", "split256map", "M%128"], env={"SRCFD_NO_GEMM32_BIG": "1"})
    add("gemm32_big_4", *big4, ["step:big:4", "M%128", "big:short_slab"])
    add("gemm32_big_4_off", *big4, ["step:group", "group:mixed", "group:nb4:bkt16:vec1", "M%128"], env={"SRCFD_NO_GEMM32_BIG": "1"})
    add("dense_skinny32", *skinny, ["step:skinny", "M%128", "skinny:short_k"])
    add("dense_skinny32_off", *skinny, ["step:mfma", "M%128"], env={"SRCFD_NO_DENSE_SKINNY": "1"})
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# what the table must reach between its cases (the issue's list; `npad` and `ci4` are not reachable by a layer graph, see above)
WANT = set()
WANT |= {f"{form}:nb{nb}:bkt{bkt}:vec{vec}" for form in ("single", "group") for nb in (1, 2, 4) for bkt in (16, 32) for vec in (0, 1)}
WANT |= {"M<128", "M=129", "M%128", "K%bkt", "K<16", "ci%4,K>32", "s2same:odd", "s2same:even", "nphx2", "nphx3"} | {f"N={n}" for n in EDGE_N}
WANT |= {"split144:short", "split256dense:short", "split256map", "finish8", "finish1:32slabs", "fin_partial:1", "fin_partial:8", "fin_partial:group"}
WANT |= {"group:count2", "group:count3", "group:count4", "group:convt3x3s2", "group:convt4x4s2", "group:same3x3s2", "group:rows_differ", "group:nosplit",
         "group:allsplit", "group:mixed", "nogroup:finish8", "nogroup:member"}
WANT |= {"tiled_n1:1x1", "tiled_n1:15x63", "tiled_n1:17x65", "tiled_n1:16x64", "n1x4", "n1", "n1:K=512", "n1:K=513", "N=1,K>512", "convt:n1"}
WANT |= {f"ci1:N={n}:{'same' if n % 2 == 0 else 'valid'}" for n in range(2, 9)}
WANT |= {f"act:{site}:{a}" for site in ("mfma", "finish", "groupfinish", "n1", "n1x4", "tiled_n1", "ci1") for a in ACTS} | {f"loop:nb{nb}" for nb in (1, 2, 4)}
WANT |= {"probe:mfma", "probe:n1"}
WANT |= {"step:big:1", "step:big:4", "step:skinny", "step:mfma", "step:group", "big:short_slab", "skinny:short_k"}


# ---------------------------------------------------------------------------------------------------------------------------------
# the graphs as the harness and the engine take them
# ---------------------------------------------------------------------------------------------------------------------------------
def forms_text(cases=None):
    """the list tools/pack_digest.cpp --forms reads (of this table, or of another one of `Case`s: tests/x3_forms.py)"""
    eng = importlib.import_module("sr-for-cfd_amd.engine")
    out = []
    for c in CASES if cases is None else cases:
        out.append(f"case {c.name} {c.batch} {c.in_shape[0]} {c.in_shape[1]} {c.in_shape[2]} {len(c.layers)}")
        for l in c.layers:
            out.append(f"layer {eng._KIND[l['kind']]} {eng._ACT[l['act']]} {l['kh']} {l['kw']} {l['stride']} {int(l['same'])} {l['cin']} {l['cout']}")
    return "\n".join(out) + "\n"


def _seed(case):
    return int.from_bytes(case.name.split("_off")[0].encode(), "little") % (2 ** 32)   # the arms of a switch share their numbers


def specs(case, with_weights=True):
    """`SRModel.from_layers` dicts; the layer under test is named `under_test`"""
    rng = np.random.default_rng(_seed(case))
    out = []
    for i, l in enumerate(case.layers):
        s = dict(kind=l["kind"], k=l["kh"], stride=l["stride"], same=l["same"], act=l["act"], name="under_test" if i == len(case.layers) - 1 else f"front{i}")
        if l["kind"] != "flatten" and with_weights:
            shape = {"conv2d": (l["kh"], l["kw"], l["cin"], l["cout"]), "conv2d_transpose": (l["kh"], l["kw"], l["cout"], l["cin"]), "dense": (l["cin"], l["cout"])}[l["kind"]]
            if l["exact"]:
                s["w"] = (rng.integers(-8, 9, shape) / 8.0).astype(np.float32)
                s["b"] = (rng.integers(-8, 9, l["cout"]) / 8.0).astype(np.float32)
            else:
                taps = l["kh"] * l["kw"] if l["kind"] == "conv2d" else -(-l["kh"] // l["stride"]) * -(-l["kw"] // l["stride"])
                s["w"] = (rng.standard_normal(shape) / np.sqrt(max(1, taps * l["cin"]))).astype(np.float32)
                s["b"] = (0.1 * rng.standard_normal(l["cout"])).astype(np.float32)
        out.append(s)
    return out


def inputs(case):
    rng = np.random.default_rng(_seed(case) + 1)
    shape = (case.batch,) + case.in_shape
    if case.layers[0]["exact"]:
        return (np.clip(np.round(rng.standard_normal(shape) * 8), -32, 32) / 16.0).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# references and the statistic
# ---------------------------------------------------------------------------------------------------------------------------------
Reference = namedtuple("Reference", "x T S q_cpu cpu32")


def _abs_layer(s):
    return dict(s, w=np.abs(np.asarray(s["w"], np.float64)), b=np.abs(np.asarray(s["b"], np.float64)), act="linear")


def layer_input64(sp, x):
    """float64 input of the layer under test (what the exact front layers leave)"""
    import family_ref
    return family_ref.forward_specs64(sp[:-1], x)


def reference(case, sp=None, x=None):
    """x, T and S of the layer under test in float64, and the float32 CPU evaluation (torch) with its q"""
    import family_ref
    import torch
    sp = specs(case) if sp is None else sp
    x = inputs(case) if x is None else x
    h = layer_input64(sp, x)
    T = family_ref.forward_specs64(sp[-1:], h)
    S = family_ref.forward_specs64([_abs_layer(sp[-1])], np.abs(h))
    sp32 = [q for i, s in enumerate(sp) for q in ([dict(kind="flatten"), s] if s["kind"] == "dense" and (i == 0 or sp[i - 1]["kind"] != "flatten") else [s])]   # the torch forward wants its Dense input flat
    params = {i: (torch.tensor(np.asarray(s["w"])), torch.tensor(np.asarray(s["b"]))) for i, s in enumerate(sp32) if "w" in s}
    with torch.no_grad():
        cpu32 = family_ref._forward_torch(sp32, params, x, torch.float32).numpy().reshape(T.shape)
    return Reference(x, T, S, statistic(cpu32, T, S), cpu32)


def q_map(y, T, S):
    """q_i; an element whose sums are all zero must be met exactly"""
    err = np.abs(np.asarray(y, np.float64).reshape(T.shape) - T)
    den = S + np.abs(T)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(q), np.inf, q)   # a NaN on either side is a miss


def statistic(y, T, S):
    return float(q_map(y, T, S).max())


def bound(q_cpu, act="linear", act_error=0.0):
    """MARGIN x max(q_cpu, floor); act_error: the device activation's own measured error (0 for linear)"""
    return MARGIN * max(q_cpu, TINY + (0.0 if act == "linear" else act_error))


def accepts(y, ref, act="linear", act_error=0.0):
    return statistic(y, ref.T, ref.S) <= bound(ref.q_cpu, act, act_error)
