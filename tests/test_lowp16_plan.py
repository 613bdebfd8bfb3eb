"""The 16-bit forward's chunk plan on a CPU (csrc/lowp16_plan.cpp: what a chunk of c samples of a graph launches -- kernels, the ops
they cover, activation buffers, M, gemm16's cut, every grid, mid16's shape and workgroup counts, the tail's segmentation -- which
csrc/fused_bf16.hip issues step by step).  The output digests of tests/test_gpu_lowp16_bits.py cannot see a wrong grid rounding, a
wrong segmentation or a split that was dropped (they cost speed or capacity, not bits); this test can.  The sanitizer-built harness
tools/pack_digest.cpp --lowp16 writes the plan of sixteen graphs -- encoder_10 + decoder_400 (the fused graph), the five other family
decoders behind encoder_10, all ten cases of tests/any16_cases.py (every one: the harness builds graphs from a layer list, not from
saved .h5 files) and one hand-written graph whose Dense layer is too wide for split-K -- at every batch, CU count and switch set
below; the checks compare every field of every step with tests/lowp16_plan_ref.py, the statement of the rules as they stood in
fused_bf16.hip and the launchers before the plan was factored out of them."""
import importlib
import os
import subprocess

import pytest

import any16_cases as ac
import lowp16_plan_ref as ref
from conftest import ROOT

FIELDS = "M N K Npad MH MW TY TX CI IH IW ay by cy ax bx cx CO nphx OH OW OC os oy0 ox0 act".split()
FUSED_BATCHES = (1, 3, 7, 64, 216, 256, 257, 768, 1024)
ANY16_BATCHES = ac.BATCHES + (67, 259)
CUS = (256, 64)
# the harness's switch sets, in its order: what Switches::from_env makes of the named environment
SETS = [("default", {}), ("SRCFD_ENC=0", dict(enc16=False)), ("SRCFD_DENSE1=0", dict(dense1_16=False)), ("SRCFD_MID=0", dict(mid16=False)),
        ("SRCFD_MID=1", dict(mid_shape=1)), ("SRCFD_MID=2", dict(mid_shape=2)), ("SRCFD_MID_WAVES=4", dict(mid_waves=4)),
        ("SRCFD_MID_WAVES=16", dict(mid_waves=16)), ("SRCFD_TAIL=s", dict(tail16s=True)), ("SRCFD_TAIL_SEG=1", dict(tail_seg=1)),
        ("SRCFD_TAIL_SEG=5", dict(tail_seg=5))]
FAMILY = (10, 20, 50, 80, 100)
GUARD = "dense_4096_to_384"     # splits * Npad = 16 * 384 > 2048: the slab guard bites at every chunk
NO_CUT = dict(bn=0, splits=1, kslice=0, nz=1, grid=(0, 0, 0), fin=0, slab=0)


def graph_text(name, specs):
    """one graph of the list tools/pack_digest.cpp --lowp16 reads, from `SRModel.from_layers` specs (the shapes only)"""
    eng = importlib.import_module("sr-for-cfd_amd.engine")
    lines = []
    for s in specs:
        kind, act = eng._KIND[s["kind"]], eng._ACT[s.get("act")]
        if s["kind"] == "flatten":
            lines.append(f"layer {kind} 0 1 1 1 0 0 0")
        elif s["kind"] == "reshape":
            lines.append(f"layer {kind} 0 1 1 1 {s['shape'][0]} {s['shape'][1]} {s['shape'][2]}")
        elif s["kind"] == "dense":
            lines.append(f"layer {kind} {act} 1 1 1 0 {s['w'].shape[0]} {s['w'].shape[1]}")
        else:
            kh, kw, a, b = s["w"].shape
            cin, cout = (b, a) if s["kind"] == "conv2d_transpose" else (a, b)
            lines.append(f"layer {kind} {act} {kh} {kw} {s['stride']} {int(s['same'])} {cin} {cout}")
    return "\n".join([f"case {name} 0 10 10 1 {len(lines)}"] + lines) + "\n"


def guard_specs(enc_weights):
    """encoder_10 + dense_1 (50 -> 4096) + a Dense 4096 -> 384 + Reshape (2, 3, 64) + a 2x2 transposed convolution + the output convolution"""
    import numpy as np
    fam = importlib.import_module("sr-for-cfd_amd.family")
    z = lambda *shape: np.zeros(shape, np.float32)
    return fam.encoder_specs(enc_weights, 10) + [
        dict(kind="dense", name="dense_1", act="swish", w=z(50, 4096), b=z(4096)), dict(kind="dense", name="dense_2", act="swish", w=z(4096, 384), b=z(384)),
        dict(kind="reshape", name="reshape", shape=(2, 3, 64)), dict(kind="conv2d_transpose", name="up", k=2, stride=2, same=False, act="swish", w=z(2, 2, 16, 64), b=z(16)),
        dict(kind="conv2d", name="out", k=3, stride=1, same=True, act="linear", w=z(3, 3, 16, 1), b=z(1))]


def all_graphs(enc_weights):
    """{name: specs}: the fused graph, the family, the any16 cases, the hand-written layer"""
    fam = importlib.import_module("sr-for-cfd_amd.family")
    graphs = {f"decoder_{hr}": fam.layers_from_weights(enc_weights, fam.synthetic_decoder_weights(hr)) for hr in (400,) + FAMILY}
    graphs.update({case: ac.build_specs(case, enc_weights, ac.random_decoder(case)) for case in ac.CASES})
    graphs[GUARD] = guard_specs(enc_weights)
    return graphs


def read_dump(path):
    """{graph: dict(fused, enc_ok, out_hw, ops=[dict(layer, Kpad, d)], chunks={(set, cus, c): dict(steps, t1_buf, tail_seg, slab, reserve)})}"""
    graphs, g, ch = {}, None, None
    for line in open(path):
        kind, *v = line.split()
        if kind == "G":
            g = graphs[v[0]] = dict(fused=bool(int(v[1])), enc_ok=bool(int(v[2])), out_hw=(int(v[3]), int(v[4])), nops=int(v[5]), ops=[], chunks={})
            continue
        v = [int(x) for x in v]
        if kind == "Q":
            assert v[0] == len(g["ops"]) and len(v) == 3 + len(FIELDS)
            g["ops"].append(dict(layer=v[1], Kpad=v[2], d=dict(zip(FIELDS, v[3:]))))
        elif kind == "C":
            ch = g["chunks"][(v[0], v[1], v[2])] = dict(nsteps=v[3], t1_buf=v[4], tail_seg=v[5], slab=v[6], reserve=v[7], steps=[])
        else:
            assert kind == "S" and len(v) == 23 + len(FIELDS)
            k = ref.KERNELS[v[0]]
            buf = lambda b: {-1: "x", -2: "y"}.get(b, b)
            st = dict(kernel=k, ops=list(range(v[1], v[1] + v[2])), src=buf(v[3]), dst=buf(v[4]))
            cut = dict(bn=v[5], splits=v[6], kslice=v[7], nz=v[8], grid=tuple(v[9:12]), fin=v[12], slab=v[13])
            grid, shape, nblk, seg, blocks, d = tuple(v[14:16]), v[16], tuple(v[17:21]), v[21], v[22], dict(zip(FIELDS, v[23:]))
            # what a kernel does not take stays at its default
            assert (k == "gemm16") or cut == NO_CUT, line
            assert (k in ("dense1_16", "gemm16", "gemm16n")) or not any(d.values()), line
            assert (k == "mid16") or (nblk == (0, 0, 0, 0) and ref.SHAPES[shape] == "w4x2"), line
            assert (k in ("tail16", "tail16s")) or (seg, blocks) == (0, 0), line
            assert (k in ("enc_conv1_16", "enc16", "dense1_16", "gemm16n", "outconv16")) or grid == (0, 0), line
            if k == "gemm16":
                st.update(cut=cut, d=d)
            elif k == "gemm16n":
                st.update(grid=grid, d=d)
            elif k == "dense1_16":
                assert grid[1] == 0
                st.update(grid=grid[:1], d=d)
            elif k == "mid16":
                st.update(shape=ref.SHAPES[shape], nblk=nblk)
            elif k in ("tail16", "tail16s"):
                st.update(seg=seg, blocks=blocks)
            else:
                assert grid[1] == 0
                st.update(grid=grid[:1])
            ch["steps"].append(st)
    for g in graphs.values():
        assert len(g["ops"]) == g["nops"] and all(len(c["steps"]) == c["nsteps"] for c in g["chunks"].values())
    return graphs


def dump_plans(srcfd_unused, enc_weights, tmp):
    """one sanitizer-clean run of the harness over all_graphs -> read_dump's dict"""
    lst = tmp / "graphs.txt"
    lst.write_text("".join(graph_text(name, specs) for name, specs in all_graphs(enc_weights).items()))
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sr-for-cfd_amd", "csrc"), "pack_digest"], stdout=subprocess.DEVNULL)
    dump = tmp / "dump"
    dump.mkdir()
    out = subprocess.run([os.path.join(ROOT, "sr-for-cfd_amd", "lib", "pack_digest_asan"), "--lowp16", str(lst), str(dump)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]   # ASan / UBSan clean
    return read_dump(str(dump / "lowp16.plan.txt"))


_PLANS = {}


@pytest.fixture(scope="session")
def lowp16_plans(srcfd, enc_weights, tmp_path_factory):
    if not _PLANS:
        _PLANS.update(dump_plans(srcfd, enc_weights, tmp_path_factory.mktemp("lowp16_plan")))
    return _PLANS


def switches(i):
    return dict(ref.DEFAULT, **SETS[i][1])


def every(plans):
    return [(name, g, key, ch) for name, g in plans.items() for key, ch in g["chunks"].items()]


def test_the_dump_covers_the_graphs_batches_and_switches(lowp16_plans):
    assert set(lowp16_plans) == {f"decoder_{hr}" for hr in (400,) + FAMILY} | set(ac.CASES) | {GUARD}
    for name, g in lowp16_plans.items():
        assert g["fused"] == (name == "decoder_400") and g["enc_ok"] == g["fused"], name
        batches = FUSED_BATCHES if g["fused"] else ANY16_BATCHES
        assert set(g["chunks"]) == {(s, cus, c) for s in range(len(SETS)) for cus in CUS for c in batches}, name
        if name in ac.CASES:
            assert g["out_hw"] == ac.out_hw(name)
    assert len(lowp16_plans["decoder_400"]["ops"]) == 9


def test_every_step_matches_the_reference(lowp16_plans):
    for name, g, (s, cus, c), ch in every(lowp16_plans):
        steps, t1_buf, seg = ref.chunk(g["ops"], g["fused"], g["enc_ok"], g["out_hw"], switches(s), c, cus)
        where = (name, SETS[s][0], cus, c)
        assert len(ch["steps"]) == len(steps), where
        for got, want in zip(ch["steps"], steps):
            assert got == want, (where, got, want)
        assert (ch["t1_buf"], ch["tail_seg"]) == ((t1_buf, seg) if g["fused"] else (0, 0)), where
        assert ch["slab"] == max([st["cut"]["slab"] for st in steps if st["kernel"] == "gemm16"] + [0]), where


def test_tail_segmentation_worked_by_hand(lowp16_plans):
    """At 256 CUs, from the cost rule (strips walked by the busiest workgroup, 15 % bar): 1 sample: 52 -> S = 25: 1 x 3 + 2 = 5.
    64 samples: S = 10: ceil(640 / 256) = 3 virtual samples of 6 strips + 2 = 20 beats S = 25: 7 x 3 + 2 = 23.  257 samples: 102 ->
    S = 5: 6 x 11 + 2 = 68 (S = 10: 11 x 6 + 2 = 68 is no 15 % better).  768 samples: 152, S = 2: 6 x 26 + 2 = 158: no cut."""
    chunks = lowp16_plans["decoder_400"]["chunks"]
    for c, seg in ((1, 25), (3, 25), (7, 25), (64, 10), (257, 5), (768, 1)):
        ch = chunks[(0, 256, c)]
        assert ch["tail_seg"] == seg == ch["steps"][-1]["seg"] == ref.tail_seg(ref.DEFAULT, c, 256), c
        assert ch["steps"][-1]["blocks"] == min(c * seg, 256)
    assert {chunks[(0, 64, c)]["tail_seg"] for c in FUSED_BATCHES} > {1}          # both sides of "fewer samples than CUs" on the small chip too
    assert chunks[(0, 64, 64)]["tail_seg"] == 1 and chunks[(0, 64, 7)]["tail_seg"] == 25
    for s, forced in ((9, 1), (10, 5)):
        assert {chunks[(s, cus, c)]["tail_seg"] for cus in CUS for c in FUSED_BATCHES} == {forced}


def test_buffers_alternate_and_layers_share_theirs(lowp16_plans):
    for name, g, key, ch in every(lowp16_plans):
        steps = ch["steps"]
        assert steps[0]["src"] == "x" and steps[-1]["dst"] == "y", (name, key)
        assert all(st["src"] in (0, 1) for st in steps[1:]) and all(st["dst"] in (0, 1) for st in steps[:-1]), (name, key)
        layer_of = lambda st: g["ops"][st["ops"][0]]["layer"] if st["kernel"] in ("dense1_16", "gemm16", "gemm16n") else id(st)
        wrote = steps[0]["dst"]
        for i in range(1, len(steps)):
            st = steps[i]
            if layer_of(st) == layer_of(steps[i - 1]):                           # the output phases of one transposed convolution
                assert (st["src"], st["dst"]) == (steps[i - 1]["src"], steps[i - 1]["dst"]), (name, key, i)
                continue
            assert st["src"] == wrote, (name, key, i)                            # every step reads what the previous layer wrote
            if st["dst"] != "y":
                assert st["dst"] == st["src"] ^ 1, (name, key, i)
                wrote = st["dst"]
        if g["fused"]:
            assert ch["t1_buf"] == steps[-1]["src"]
        # every op is covered exactly once, in order
        covered = [i for st in steps for i in st["ops"]]
        assert covered == list(range(len(g["ops"]))), (name, key)


def test_the_fused_graph_is_four_launches_by_default(lowp16_plans):
    for (s, cus, c), ch in lowp16_plans["decoder_400"]["chunks"].items():
        kernels = [st["kernel"] for st in ch["steps"]]
        if SETS[s][0] in ("default", "SRCFD_TAIL_SEG=1", "SRCFD_TAIL_SEG=5"):
            assert kernels == ["enc16", "dense1_16", "mid16", "tail16"]
            assert ch["steps"][2]["shape"] == "w4x2" and ch["steps"][1]["grid"] == (256,)
        if SETS[s][0] == "SRCFD_ENC=0":
            assert kernels == ["enc_conv1_16", "gemm16", "gemm16", "gemm16", "dense1_16", "mid16", "tail16"]
            assert ch["steps"][2]["cut"]["splits"] == 12 and ch["steps"][2]["cut"]["nz"] == 10            # dense, K = 3200: 12 asked, 10 slabs of 320
        if SETS[s][0] == "SRCFD_MID=0":
            assert kernels == ["enc16", "dense1_16"] + ["gemm16"] * 5 + ["tail16"]
        if SETS[s][0] == "SRCFD_DENSE1=0":
            assert kernels == ["enc16", "gemm16", "mid16", "tail16"]
        if SETS[s][0] == "SRCFD_TAIL=s":
            assert kernels[-1] == "tail16s"
    shapes = {SETS[s][0]: ch["steps"][2]["shape"] for (s, cus, c), ch in lowp16_plans["decoder_400"]["chunks"].items() if SETS[s][0] != "SRCFD_MID=0" and s != 1}
    assert shapes["SRCFD_MID=1"] == "w8" and shapes["SRCFD_MID=2"] == "w8x2" and shapes["SRCFD_MID_WAVES=4"] == "w4" and shapes["SRCFD_MID_WAVES=16"] == "w16"


def test_the_reserve_holds_every_plan_and_the_guard_never_bites(lowp16_plans):
    """lowp16_reserve sizes the slabs 16 x chunk x 128 floats for the largest chunk of a call, and a chunk is never larger than that:
    every plan's slab need is within the reserve of its own chunk, so the launcher never meets a split cut without slabs.  On every
    shipped or tested graph a layer eligible for split-K has splits * Npad <= 2048 and is split; on the hand-written Dense
    4096 -> 384 it is not, at any chunk."""
    eligible = 0
    for name, g, (s, cus, c), ch in every(lowp16_plans):
        assert ch["reserve"] == 16 * c * 128 and ch["slab"] <= ch["reserve"], (name, s, cus, c)
        for st in ch["steps"]:
            if st["kernel"] != "gemm16":
                continue
            d = st["d"]
            if d["OH"] == d["OW"] == d["MH"] == d["MW"] == 1 and d["K"] >= 1024:
                asked = max(1, min(16, d["K"] // 256))
                if name == GUARD and d["K"] == 4096:
                    assert asked * d["Npad"] > 2048 and st["cut"]["splits"] == 1 and st["cut"]["nz"] == 1 and st["cut"]["slab"] == 0, (s, cus, c)
                else:
                    assert asked * d["Npad"] <= 2048 and st["cut"]["splits"] == asked, (name, s, cus, c)
                    eligible += 1
            else:
                assert st["cut"]["splits"] == 1
    assert eligible > 0
    assert any(st["kernel"] == "gemm16" and st["cut"]["splits"] > 1 for st in lowp16_plans["mid_dense_splitk"]["chunks"][(0, 256, 130)]["steps"])
    # what the parent commit did on a handle that had seen a larger chunk: the guarded layer split 16 ways.  The reference with the
    # old buffer (1024-sample reserve) shows the history dependence the plan no longer has
    g = lowp16_plans[GUARD]
    old = ref.chunk(g["ops"], False, False, g["out_hw"], ref.DEFAULT, 3, 256, slab_elems=16 * 1024 * 128)[0]
    assert [st["cut"]["splits"] for st in old if st["kernel"] == "gemm16" and st["d"]["K"] == 4096] == [16]
