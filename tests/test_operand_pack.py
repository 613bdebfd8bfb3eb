"""The host-side operand packers (sr-for-cfd_amd/csrc/operand_pack.cpp) on a CPU: every blob a kernel reads its weights from, hashed by
the sanitizer-built harness tools/pack_digest.cpp and compared with tests/golden/operand_pack_digests.json -- the digests of the host
buffers commit 166b6e2 handed to its host-to-device copies (tests/golden/record_operand_digests.py).  A wrong index in a pack is a
swapped channel or lattice phase on the device; here it is a section name."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

LOG2E = 1.4426950408889634
SCALES = (1.0, LOG2E, 1.0 / LOG2E)

REQUIRED = (
    ["pack", "ops_off", "plan", "pack.enc32_w2", "pack_x3", "x3_off", "pack_x3.t32_w1x", "pack_x3.t32_w2x"]
    + ["pack.pair_" + s for s in ("wa", "ba", "wb", "bb")]
    + ["pack.tri_" + s for s in ("w1", "b1", "w2", "b2", "w3", "b3")]
    + ["pack.t32_" + s for s in ("w1", "b1", "w2", "b2", "w3", "b3", "wc")]
    + ["fused.f32", "fused.b_off", "fused.c1_off"]
    + [p + s for p in ("bf16.", "f16.") for s in ("Wt", "w_off", "encf", "enc_off", "encb", "consts", "w2f", "w1f", "w0t", "w0t_off", "midb")]
    + ["train.map", "train.scale", "train.tail_map", "train.tail_gmap", "train.tail_plan", "train.init_params", "train.offsets", "train.dops_off"]
    + [f"train.op{i}.gmap" for i in range(14)]
    # the harness's own graphs: a 3x3 stride-2 ConvT (four phases), 32 -> 16 -> 8 without 64 -> 32 in front, an encoder enc32 declines
    + ["convt3.pack", "convt3.ops_off", "convt3.plan", "pair.pack", "pair.plan", "noenc32.pack", "noenc32.plan"]
    + ["pair.pack.pair_" + s for s in ("wa", "ba", "wb", "bb")]
)


@pytest.fixture(scope="module")
def run(srcfd, enc_weights, tmp_path_factory):
    """One run of the harness on the trained multiBC encoder + the synthetic decoder: (sections by name, directory of raw arrays)."""
    tmp = tmp_path_factory.mktemp("operand_pack")
    h5 = str(tmp / "superres.h5")
    synth = importlib.import_module("sr-for-cfd_amd.synth")
    srcfd.SRModel.from_weights(enc_weights, synth.synthetic_decoder_weights(1), device=-1).save_superres_h5(h5)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sr-for-cfd_amd", "csrc"), "pack_digest"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "sr-for-cfd_amd", "lib", "pack_digest_asan")
    dump = tmp / "dump"
    dump.mkdir()
    out = subprocess.run([exe, h5, str(dump)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]   # ASan / UBSan clean
    return {s["name"]: s for s in json.loads(out.stdout)["sections"]}, str(dump)


def test_every_packer_is_reached(run):
    missing = [n for n in REQUIRED if n not in run[0]]
    assert not missing, f"sections the harness did not produce: {missing}"


def test_sections_match_the_recorded_digests(run):
    golden = json.load(open(os.path.join(GOLDEN, "operand_pack_digests.json")))["sections"]
    missing = [n for n in REQUIRED if n not in golden]
    assert not missing, f"sections without a recorded digest: {missing}"
    assert sorted(golden) == sorted(run[0]), sorted(set(golden) ^ set(run[0]))
    bad = [n for n, g in golden.items() if (run[0][n]["off"], run[0][n]["len"], run[0][n]["sha256"]) != (g["off"], g["len"], g["sha256"])]
    assert not bad, f"operand sections that differ from the recorded bytes / offsets: {bad}"


def test_convt3_plans_four_phases(run):
    assert run[0]["convt3.ops_off"]["len"] == 2 * 4          # (w_off, b_off) of four output phases
    assert "convt3.pack.pair_wa" not in run[0] and "pair.pack.tri_w1" not in run[0] and "noenc32.pack.enc32_w2" not in run[0]


def test_trainer_tail_map_reproduces_the_inference_sections(run):
    """float32(float64(params[map - 1]) * s), s named by the scale vector, is the engine's tail32 section bit for bit; the stored
    scale is float32(s) and unmapped slots are 0."""
    sec, dump = run
    params = np.fromfile(os.path.join(dump, "train.init_params.bin"), np.float32)
    tmap = np.fromfile(os.path.join(dump, "train.tail_map.bin"), np.int32)
    scale = np.fromfile(os.path.join(dump, "train.scale.bin"), np.float32)
    pack = np.fromfile(os.path.join(dump, "pack.bin"), np.float32)
    assert tmap.shape == scale.shape and tmap.min() == 0 and tmap.max() <= params.size
    klass = np.full(scale.shape, -1)
    for i, s in enumerate(SCALES):
        klass[scale == np.float32(s)] = i
    assert (klass[tmap > 0] >= 0).all(), "a scale that is none of 1, log2(e), 1 / log2(e)"
    assert (scale[tmap == 0] == 0).all()
    want = np.where(tmap > 0, (params[np.maximum(tmap, 1) - 1].astype(np.float64) * np.asarray(SCALES)[np.maximum(klass, 0)]).astype(np.float32), np.float32(0))
    lo, hi = sec["pack.t32_w1"]["off"], sec["pack.t32_wc"]["off"] + 128     # t32_w1 .. the padded end of t32_wc
    n = hi - lo
    got = pack[lo:hi]
    assert n == 8192 + 64 + 2048 + 64 + 512 + 64 + 128
    assert want[:n].tobytes() == got.tobytes(), f"first differing slot {int(np.flatnonzero(want[:n].view(np.uint32) != got.view(np.uint32))[0])}"


def test_trainer_gmaps_are_bijections(run):
    """Every weight-gradient map sends the non-pad slots of a layer's ops one to one onto the layer's parameters; only the bias of a
    merged-phase ConvT (nphx > 1: one GEMM column per output phase) is hit more than once, once per phase."""
    sec, dump = run
    ops = np.loadtxt(os.path.join(dump, "train.ops.txt"), dtype=np.int64)   # K N Npad layer nphx
    by_layer = {}
    for i, (K, N, Npad, layer, nphx) in enumerate(ops):
        g = np.fromfile(os.path.join(dump, f"train.op{i}.gmap.bin"), np.int32).reshape(K + 1, Npad)
        assert (g[:, N:] == 0).all() and (g[:, :N] > 0).all(), f"train.op{i}.gmap: padding"
        w = g[:K, :N].ravel()
        assert np.unique(w).size == w.size, f"train.op{i}.gmap: a weight mapped twice"
        b, counts = np.unique(g[K, :N], return_counts=True)
        assert (counts == (nphx * nphx if nphx > 1 else 1)).all(), f"train.op{i}.gmap: bias multiplicity"
        by_layer.setdefault(int(layer), []).append((w, b))
    seen = []
    for layer, parts in sorted(by_layer.items()):
        w = np.concatenate([p[0] for p in parts])
        assert np.unique(w).size == w.size, f"layer {layer}: a weight in two phases"
        for p in parts[1:]:
            assert np.array_equal(p[1], parts[0][1])          # the phases of a strided ConvT share one bias
        idx = np.sort(np.concatenate([w, parts[0][1]]))
        assert np.array_equal(idx, np.arange(idx[0], idx[0] + idx.size)), f"layer {layer}: parameters not covered exactly once"
        seen.append(idx)
    allp = np.concatenate(seen)
    assert np.array_equal(allp, np.arange(1, sec["train.init_params"]["len"] + 1))
