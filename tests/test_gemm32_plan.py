"""The f32 GEMM's launch plan on a CPU (csrc/gemm32_plan.cpp: the kernel that takes a descriptor, the split-K cut, nb / BKT / VEC,
the grouping of a layer's GEMMs, every grid and the slab floats -- what launch_gemm_mfma / launch_gemm_mfma_group issue and what
the engine and the trainer size their slab buffers from).  The output digests of tests/test_gpu_f32_forward_bits.py and
tests/test_gpu_train_step_bits.py cannot see a wrong nb or BKT (the k order is the same for any of them: it costs speed, not bits);
this test can.  The sanitizer-built harness tools/pack_digest.cpp writes the plan of the SR network, of its own small graphs, of a
family member (encoder_10 + decoder_80) and of a few hand-written layers into its dump directory, for inference at 1 .. 768 samples
and for the training step's forward and data-gradient GEMMs at 1 .. 8 and 32; the checks compare every line with
tests/gemm32_plan_ref.py, the statement of the launchers' rules as they stood before the plan was factored out of them."""
import importlib
import os
import subprocess

import pytest

from conftest import ROOT
import gemm32_plan_ref as ref

FIELDS = "M N K Npad MH MW TY TX CI IH IW ay by cy ax bx cx CO nphx OH OW OC os oy0 ox0 act".split()
TAGS = ("", "convt3.", "pair.", "noenc32.", "hand.", "family.")
BATCHES = {0: (1, 3, 7, 64, 216, 768), 1: (1, 2, 3, 4, 5, 6, 7, 8, 32), 2: (1, 2, 3, 4, 5, 6, 7, 8, 32)}   # mode: inference, training forward, data gradients


def read_plan(path):
    """launches of one dump file: dict(mode, n, first, count, grouped, launch, ws, fits, ops=[dict(plan, derived, d)])"""
    return read_plan_lines(open(path))


def read_plan_lines(lines):
    """the same of G / O lines from anywhere (tests/test_gemm32_forms.py: one case of the forms dump)"""
    launches, by_first = [], {}
    for line in lines:
        kind, *v = line.split()
        v = [int(x) for x in v]
        if kind == "G":
            g = dict(mode=v[0], n=v[1], first=v[2], count=v[3], grouped=bool(v[4]), launch=dict(nb=v[5], bkt=v[6], vec=v[7], grid=tuple(v[8:11]), fin=tuple(v[11:13])),
                     ws=v[13], fits=tuple(v[14:17]), ops=[])
            launches.append(g)
            by_first[(g["mode"], g["n"])] = g
        else:
            assert kind == "O" and len(v) == 18 + len(FIELDS)
            g = by_first[(v[0], v[1])]
            assert v[2] == g["first"] + len(g["ops"]) and len(g["ops"]) < g["count"]
            g["ops"].append(dict(plan=dict(route=ref.ROUTES[v[3]], splits=v[4], kchunk=v[5], slab_off=v[6], finish_groups=v[7], nb=v[8], bkt=v[9], vec=v[10],
                                           grid=tuple(v[11:14]), fin=v[14]),
                                 epi_aux=bool(v[15]), fuses_finalize=bool(v[16]), splitk_ws=v[17], d=dict(zip(FIELDS, v[18:]))))
    assert all(len(g["ops"]) == g["count"] for g in launches)
    return launches


@pytest.fixture(scope="module")
def plans(srcfd, enc_weights, tmp_path_factory):
    """{tag: launches} of one sanitizer-clean run of the harness"""
    tmp = tmp_path_factory.mktemp("gemm32_plan")
    base, famh5 = str(tmp / "superres.h5"), str(tmp / "superres_10to80.h5")
    dec_w = importlib.import_module("sr-for-cfd_amd.synth").synthetic_decoder_weights(1)
    srcfd.SRModel.from_weights(enc_weights, dec_w, device=-1).save_superres_h5(base)
    fam = importlib.import_module("sr-for-cfd_amd.family")
    srcfd.SRModel.from_weights(enc_weights, fam.synthetic_decoder_weights(80), device=-1).save_superres_h5(famh5)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sr-for-cfd_amd", "csrc"), "pack_digest"], stdout=subprocess.DEVNULL)
    dump = tmp / "dump"
    dump.mkdir()
    out = subprocess.run([os.path.join(ROOT, "sr-for-cfd_amd", "lib", "pack_digest_asan"), base, str(dump), famh5], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]   # ASan / UBSan clean
    return {tag: read_plan(str(dump / (tag + "gemm32.plan.txt"))) for tag in TAGS}


def every(plans):
    return [(tag, g) for tag, launches in plans.items() for g in launches]


def test_the_dump_covers_the_graphs_and_batches(plans):
    sr = plans[""]
    for mode, batches in BATCHES.items():
        assert sorted({g["n"] for g in sr if g["mode"] == mode}) == list(batches)
    fwd = [o for g in sr if (g["mode"], g["n"]) == (0, 3) for o in g["ops"]]
    assert len(fwd) == 14 and sorted(g["count"] for g in sr if (g["mode"], g["n"]) == (0, 3)) == [1] * 10 + [4]   # ConvT#0's four phases
    for tag, launches in plans.items():
        assert {g["mode"] for g in launches} == ({0, 1} if tag == "convt3." else {0, 1, 2}), tag   # a one-layer graph has no data gradient
        assert all(o["d"]["M"] == g["n"] * o["d"]["MH"] * o["d"]["MW"] for g in launches for o in g["ops"]), tag
    assert [g["count"] for g in plans["convt3."] if (g["mode"], g["n"]) == (1, 1)] == [4]


def test_every_line_matches_the_reference(plans):
    """Grouped or not, the group's launch, every op's route, cut, slab offset, finish groups and own launch, and the slab floats."""
    for tag, g in every(plans):
        inv = g["mode"] == 0
        ds = [o["d"] for o in g["ops"]]
        why, launch, ops = ref.group(ds, inv)
        where = (tag, g["mode"], g["n"], g["first"])
        assert g["grouped"] == (why is None), (where, why)
        assert g["launch"] == (launch or dict(nb=0, bkt=0, vec=0, grid=(0, 0, 0), fin=(0, 0))), where
        assert g["ws"] == sum(o["ws"] for o in ops), where
        for got, want in zip(g["ops"], ops):
            ws = want.pop("ws")
            assert got["plan"] == want, (where, got["plan"], want)
            assert got["splitk_ws"] == ws


def test_coverage(plans):
    """Every branch of the rules is reached by at least one dumped case (classified by the reference, which the test above ties to
    the library): the five kernels, nb 1 / 2 / 4 and BKT 16 / 32 in single and in grouped launches, split and unsplit, grouped, each
    way of not being grouped, both finishes."""
    seen = set()
    for tag, g in every(plans):
        ds = [o["d"] for o in g["ops"]]
        why, launch, ops = ref.group(ds, g["mode"] == 0)
        seen.add(("group", why if len(ds) > 1 else "single"))
        for o in ops:
            seen.add(("route", o["route"]))
            if o["route"] == "mfma":
                seen.add(("split", o["splits"] > 1))
                seen.add(("finish_groups", o["finish_groups"]))
                seen.add(("cut", g["mode"] == 0, o["splits"] > 1))
        for l, form in [(launch, "grouped")] + [(o, "single") for o in ops if o["route"] == "mfma"]:
            if l and l["nb"]:
                seen |= {("nb", form, l["nb"]), ("bkt", form, l["bkt"]), ("vec", l["vec"])}
    want = {("route", r) for r in ref.ROUTES[1:]} | {("group", w) for w in (None, "member", "npad", "ci4", "finish8", "single")}
    want |= {("nb", f, nb) for f in ("single", "grouped") for nb in (1, 2, 4)} | {("bkt", f, b) for f in ("single", "grouped") for b in (16, 32)}
    want |= {("split", True), ("split", False), ("finish_groups", 1), ("finish_groups", 8), ("vec", 0), ("vec", 1)}
    want |= {("cut", inv, s) for inv in (True, False) for s in (True, False)}
    assert not want - seen, sorted(want - seen, key=str)


def test_the_hand_written_layers_take_the_kernels_they_were_written_for(plans):
    routes = [o["plan"]["route"] for g in plans["hand."] if (g["mode"], g["n"]) == (0, 3) for o in g["ops"]]   # file order
    assert routes[:7] == ["n1x4", "n1", "ci1", "n1", "n1", "n1", "n1"]   # 8 -> 1 not SAME; 3 -> 1; 1 -> 4; a 4 -> 1 ConvT's phases
    assert routes[7:] == ["mfma"] * 12
    sr_out = [g for g in plans[""] if (g["mode"], g["n"]) == (0, 3)][-1]
    assert sr_out["ops"][0]["plan"]["route"] == "tiled_n1" and sr_out["ops"][0]["plan"]["grid"] == (7, 25, 3)   # 400 x 400: 64 x 16 pixel tiles


def test_derived_answers(plans):
    for tag, g in every(plans):
        for o in g["ops"]:
            r = o["plan"]["route"]
            assert o["epi_aux"] == (r in ("mfma", "ci1")), (tag, o)
            assert o["fuses_finalize"] == (r == "tiled_n1"), (tag, o)
            if r != "mfma":
                assert o["splitk_ws"] == 0 and o["plan"]["splits"] == 1, (tag, o)
            else:
                assert o["splitk_ws"] == (o["plan"]["splits"] * o["d"]["M"] * o["d"]["Npad"] if o["plan"]["splits"] > 1 else 0)


def test_slabs_of_a_group_do_not_overlap(plans):
    for tag, g in every(plans):
        if not g["grouped"]:
            assert all(o["plan"]["slab_off"] == 0 for o in g["ops"])
            continue
        end = 0
        for o in g["ops"]:
            assert o["plan"]["slab_off"] == end, (tag, g["first"])
            end += o["splitk_ws"]
        assert end == g["ws"]
        assert g["launch"]["grid"][2] == sum(o["plan"]["splits"] for o in g["ops"])


def test_a_short_workspace_is_refused(plans):
    """gemm32_ws_fits, the one question both launchers ask before they launch anything: no for a float less than the plan needs,
    yes for what it needs, and yes for a null workspace exactly when it needs none."""
    needs = set()
    for tag, g in every(plans):
        less, exact, null = g["fits"]
        assert exact == 1, (tag, g["first"])
        assert less == (0 if g["ws"] else -1), (tag, g["first"])   # -1: nothing to take a float from
        assert null == int(g["ws"] == 0), (tag, g["first"])
        needs.add(g["ws"] > 0)
    assert needs == {True, False}
