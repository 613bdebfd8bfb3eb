"""The notebook's model family (sr-for-cfd_amd/family.py) and Conv2DTranspose(padding='same') on the host: the crop rule
against its definition, shapes and MAC counts of every member, the .h5 round trip, the training entry point and the packers
under the sanitizer harness.  The device side is tests/test_gpu_model_family.py."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import family_ref as fr
from conftest import ROOT

KS = [(3, 2), (2, 2), (3, 1), (4, 2), (5, 2)]


def _family():
    return importlib.import_module("sr-for-cfd_amd.family")


@pytest.mark.parametrize("k,s", KS)
def test_crop_rule_equals_the_autograd_definition(k, s):
    """family_ref.convt_same (VALID result, rows [pb, pb + in s)) against the input-gradient of a SAME forward convolution, in
    float64: the two are sums of the same products, so the difference is rounding at most (1e-13 on O(1) values; a wrong crop
    moves whole rows, O(1))."""
    rng = np.random.default_rng(10 * k + s)
    shapes = [(h, 3) for h in range(1, 7)] + [(4, 7), (5, 2)]
    for h, w in shapes:
        x = rng.standard_normal((2, h, w, 3))
        wt = rng.standard_normal((k, k, 4, 3))
        got = fr.convt_same(x, wt, np.zeros(4), s)
        want = fr.convt_same_definition(x, wt, s)
        assert got.shape == want.shape == (2, h * s, w * s, 4)
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (k, s, h, w)


def test_k3s2_drops_the_last_row_not_the_first():
    """pb = 0 for k = 3, s = 2: out[0, 0] holds tap (0, 0) of pixel (0, 0); torch's padding=1, output_padding=1 would drop it."""
    x = np.zeros((1, 2, 2, 1))
    x[0, 0, 0, 0] = 1.0
    w = np.zeros((3, 3, 1, 1))
    w[0, 0, 0, 0] = 5.0
    y = fr.convt_same(x, w, np.zeros(1), 2)
    assert y.shape == (1, 4, 4, 1) and y[0, 0, 0, 0] == 5.0 and np.count_nonzero(y) == 1
    x[:] = 0
    x[0, 1, 1, 0] = 1.0
    w[:] = 0
    w[2, 2, 0, 0] = 5.0
    assert np.count_nonzero(fr.convt_same(x, w, np.zeros(1), 2)) == 0   # lands at (4, 4): cropped


def test_every_submodel_has_the_notebooks_shapes_and_macs(srcfd):
    fam = _family()
    assert fam.DIMS == (10, 20, 50, 80, 100, 400)
    for lr in fam.DIMS:
        w = fam.synthetic_encoder_weights(lr)
        m = srcfd.SRModel.from_weights(w, None, device=-1, lr_dim=lr)
        assert m.input_shape == (lr, lr, 1) and m.output_shape == (1, 1, 50)
        assert m.macs_per_sample == fr.macs(fam.encoder_specs(w, lr), (lr, lr, 1))
        assert [d["name"] for d in m.layers()] == fam.layer_names(lr, None)
    for hr in fam.DIMS:
        w = fam.synthetic_decoder_weights(hr)
        m = srcfd.SRModel.from_weights(None, w, device=-1)
        assert m.input_shape == (1, 1, 50) and m.output_shape == (hr, hr, 1) and fam.output_dim(hr) == hr
        assert m.macs_per_sample == fr.macs(fam.decoder_specs(w), (1, 1, 50))
        assert [d["name"] for d in m.layers()] == fam.layer_names(None, hr)
        assert {k: v.shape for k, v in w.items() if k.endswith("/kernel")} == {f"{n}/kernel": s for n, s in fam.decoder_shapes(hr).items()}


@pytest.mark.parametrize("hr", [10, 20, 50, 80, 100, 400])
def test_encoder10_plus_every_decoder(srcfd, enc_weights, hr):
    fam = _family()
    dec = fam.synthetic_decoder_weights(hr)
    specs = srcfd.layers_from_weights(enc_weights, dec)
    m = srcfd.SRModel.from_weights(enc_weights, dec, device=-1)
    assert m.input_shape == (10, 10, 1) and m.output_shape == (hr, hr, 1)
    assert m.macs_per_sample == fr.macs(specs, (10, 10, 1))
    assert [d["name"] for d in m.layers()] == fam.layer_names(10, hr)
    same = [d["same"] for d in m.layers() if d["kind"] == 2]
    assert same == [p for _, _, p in fam.DECODER_CONVTS[hr][1]]
    assert m.has_fused_path == (hr == 400)


def test_present_results_for_10_and_400_are_kept(srcfd, enc_weights, dec_weights):
    """engine.layers_from_weights and synth.py delegate to family.py and answer as before."""
    fam, synth = _family(), importlib.import_module("sr-for-cfd_amd.synth")
    specs = srcfd.layers_from_weights(enc_weights, dec_weights)
    assert [(s["kind"], s["name"], s.get("k"), s.get("stride"), s.get("same"), s.get("act"), s.get("shape")) for s in specs] == [
        ("conv2d", "conv2d", 3, 2, True, "swish", None), ("conv2d", "conv2d_1", 3, 1, True, "swish", None), ("flatten", "flatten", None, None, None, None, None),
        ("dense", "dense", None, None, None, "swish", None), ("dense", "latent_vector", None, None, None, "linear", None),
        ("dense", "dense_1", None, None, None, "swish", None), ("reshape", "reshape", None, None, None, None, (12, 12, 256)),
        ("conv2d_transpose", "conv2d_transpose", 3, 2, False, "swish", None)] + [
        ("conv2d_transpose", f"conv2d_transpose_{i}", 2, 2, False, "swish", None) for i in range(1, 5)] + [
        ("conv2d", "output_image_400", 3, 1, True, "linear", None)]
    assert list(synth.DECODER_SHAPES.items()) == [("dense_1", (50, 36864)), ("conv2d_transpose", (3, 3, 128, 256)), ("conv2d_transpose_1", (2, 2, 64, 128)),
                                                  ("conv2d_transpose_2", (2, 2, 32, 64)), ("conv2d_transpose_3", (2, 2, 16, 32)),
                                                  ("conv2d_transpose_4", (2, 2, 8, 16)), ("output_image_400", (3, 3, 8, 1))]
    assert list(synth.ENCODER_SHAPES.items()) == [("conv2d", (3, 3, 1, 64)), ("conv2d_1", (3, 3, 64, 128)), ("dense", (3200, 128)), ("latent_vector", (128, 50))]
    # the generator's draws, restated: uniform kernels then normal biases, layer by layer
    rng = np.random.default_rng(1)
    lim = np.sqrt(3.0 * 2.4 / 50)
    k = rng.uniform(-lim, lim, size=(50, 36864)).astype(np.float32)
    b = (0.1 * rng.standard_normal(36864)).astype(np.float32)
    w = synth.synthetic_decoder_weights(1)
    assert np.array_equal(w["dense_1/kernel"], k) and np.array_equal(w["dense_1/bias"], b)
    e, d = synth.keras_default_init(3)
    e2, d2 = fam.keras_default_init(10, 400, 3)
    assert all(np.array_equal(e[q], e2[q]) for q in e) and all(np.array_equal(d[q], d2[q]) for q in d)
    lim = np.sqrt(6.0 / (9 * 1 + 9 * 64))
    assert np.array_equal(e["conv2d/kernel"], np.random.default_rng(3).uniform(-lim, lim, size=(3, 3, 1, 64)).astype(np.float32))


def _one_convt(k, s, same, cin=3, cout=2, act="linear"):
    rng = np.random.default_rng(k * 7 + s)
    return [dict(kind="conv2d_transpose", name="up", k=k, stride=s, same=same, act=act, w=rng.standard_normal((k, k, cout, cin)).astype(np.float32),
                 b=rng.standard_normal(cout).astype(np.float32))]


def test_same_padding_rules_at_create(srcfd):
    with pytest.raises(ValueError, match="'up'.*smaller than the stride"):
        srcfd.SRModel.from_layers(_one_convt(2, 3, True), (4, 4, 3), device=-1)
    with pytest.raises(ValueError, match="'up'.*smaller than the stride"):
        srcfd.SRModel.from_layers(_one_convt(1, 2, True), (4, 4, 3), device=-1)
    a = srcfd.SRModel.from_layers(_one_convt(2, 2, True), (4, 5, 3), device=-1)
    b = srcfd.SRModel.from_layers(_one_convt(2, 2, False), (4, 5, 3), device=-1)
    assert a.output_shape == b.output_shape == (8, 10, 2) and a.macs_per_sample == b.macs_per_sample == 4 * 5 * 4 * 3 * 2
    for k, s in KS:
        for h, w in ((1, 1), (3, 4), (6, 5)):
            specs = _one_convt(k, s, True)
            m = srcfd.SRModel.from_layers(specs, (h, w, 3), device=-1)
            assert m.output_shape == (h * s, w * s, 2)
            assert m.macs_per_sample == fr.macs(specs, (h, w, 3))
    m = srcfd.SRModel.from_layers(_one_convt(3, 2, True), (7, 9, 3), device=-1)
    assert m.macs_per_sample == (3 * 7 - 1) * (3 * 9 - 1) * 3 * 2


def _layer_rows(m):
    return [(d["name"], d["kind"], d["kh"], d["kw"], d["stride"], d["same"], d["activation"], d["cin"], d["cout"], d["reshape"]) for d in m.layers()]


def test_h5_round_trip_of_encoder10_decoder100(srcfd, enc_weights, tmp_path):
    fam = _family()
    dec = fam.synthetic_decoder_weights(100, seed=4)
    m = srcfd.SRModel.from_weights(enc_weights, dec, device=-1)
    e, d, q = (str(tmp_path / n) for n in ("vanilla_encoder10_to_100_t.h5", "vanilla_decoder100_from_10_t.h5", "superres_10to100_vanilla_ae_t.h5"))
    m.save_h5(e, d)
    m.save_superres_h5(q)
    with srcfd.H5File(d) as f:
        cfg = json.loads(f.attr_str("/", "model_config")[0])
    pads = [(l["config"]["name"], l["config"]["padding"]) for l in cfg["config"]["layers"] if l["class_name"] == "Conv2DTranspose"]
    assert pads == [("conv2d_transpose", "same"), ("conv2d_transpose_1", "same"), ("conv2d_transpose_2", "valid"), ("conv2d_transpose_3", "valid"),
                    ("conv2d_transpose_4", "valid")]
    assert cfg["config"]["name"] == "decoder_100"
    with srcfd.H5File(q) as f:
        assert '"padding": "same"' in f.attr_str("/", "model_config")[0]
    for back in (srcfd.SRModel.load_h5(e, d, device=-1), srcfd.SRModel.load_superres_h5(q, device=-1)):
        assert _layer_rows(back) == _layer_rows(m)
        assert back.output_shape == (100, 100, 1) and back.macs_per_sample == m.macs_per_sample
        w0, w1 = m.weights(), back.weights()
        assert list(w0) == list(w1) and all(np.array_equal(w0[k], w1[k]) for k in w0)
    # the decoder file alone, through the Keras-style surface
    kc = importlib.import_module("sr-for-cfd_amd.keras_compat")
    lm = kc.load_model(d, compile=False)
    assert lm.input_shape == (None, 50) and lm.output_shape == (None, 100, 100, 1)


def test_weights_only_superres_of_another_member_is_still_refused(srcfd, enc_weights, tmp_path):
    """Layer names do not carry strides or paddings: a whole-model file without sub-model configs is accepted for the
    reference's encoder_10 / decoder_400 shapes only."""
    dec = _family().synthetic_decoder_weights(100)
    ww = srcfd.H5Writer()
    ww.attr("/", "model_config", '{"class_name": "SuperResolutionAE"}')
    ww.group("model_weights")
    ww.attr("/model_weights", "layer_names", ["encoder_10", "decoder_100"])
    for sub, ws in (("encoder_10", enc_weights), ("decoder_100", dec)):
        ww.group(f"model_weights/{sub}")
        ww.attr(f"/model_weights/{sub}", "weight_names", list(ws))
        for k, v in ws.items():
            ww.dataset(f"model_weights/{sub}/{k}", v)
    p = str(tmp_path / "superres_weights_only.h5")
    ww.save(p)
    with pytest.raises(OSError, match="architecture not recoverable"):
        srcfd.SRModel.load_superres_h5(p, device=-1)


def test_supports_precision(srcfd, enc_weights, dec_weights):
    """srcfd_model_supports_precision on host-only handles: bf16 / f16 for encoder_10 + every decoder of the family; not for an
    encoder alone, another encoder, or a graph that ends in two output channels.  set_precision agrees."""
    fam = _family()
    for hr in (10, 20, 50, 80, 100, 400):
        m = srcfd.SRModel.from_weights(enc_weights, fam.synthetic_decoder_weights(hr), device=-1)
        for p in ("bf16", "f16", "fp32", "fp32_naive", "fp32x3"):
            assert m.supports_precision(p), (hr, p)
        m.precision = "bf16"
        assert m.precision == "bf16" and m.has_fused_path == (hr == 400)
        assert m.footprint(6, "bf16")["device_workspace"] > 0
    two = dict(fam.synthetic_decoder_weights(100))
    k = two["output_image_100/kernel"]
    two["output_image_100/kernel"] = np.concatenate([k, k], axis=3)
    two["output_image_100/bias"] = np.zeros(2, np.float32)
    refused = [srcfd.SRModel.from_weights(enc_weights, None, device=-1),
               srcfd.SRModel.from_weights(fam.synthetic_encoder_weights(50), fam.synthetic_decoder_weights(100), device=-1, lr_dim=50),
               srcfd.SRModel.from_weights(enc_weights, two, device=-1)]
    assert refused[2].output_shape == (100, 100, 2)
    for m in refused:
        assert m.supports_precision("fp32") and not m.supports_precision("bf16") and not m.supports_precision("f16")
        with pytest.raises(ValueError):
            m.precision = "f16"
        with pytest.raises(ValueError):
            m.footprint(6, "bf16")


def test_train_main_builds_any_family_pair(srcfd):
    tm = importlib.import_module("sr-for-cfd_amd.train_main")
    m = tm.build_model(10, 100, 0, device=-1)
    assert m.input_shape == (10, 10, 1) and m.output_shape == (100, 100, 1)
    assert all(not d["bias"].any() for d in m.layers() if "bias" in d)          # Keras' default: zero biases
    for hr in (10, 20, 50, 80, 400):
        assert tm.build_model(10, hr, 0, device=-1).output_shape == (hr, hr, 1)
    with pytest.raises(SystemExit, match="trainable encoders"):
        tm.build_model(50, 100, 0, device=-1)
    with pytest.raises(SystemExit, match="the family defines"):
        tm.build_model(10, 200, 0, device=-1)


def _family_harness(srcfd, enc_weights, tmp_path, hr):
    """One sanitizer-clean run of tools/pack_digest.cpp on encoder_10 + decoder_400 and the family file of decoder_{hr}: (the
    family model, sections by name, directory of raw arrays).  The decoder_400 sections keep their recorded bytes; every
    `family.*` section has the offset, length and bytes recorded in tests/golden/family_pack_digests.json."""
    fam = _family()
    base, famh5 = str(tmp_path / "superres.h5"), str(tmp_path / f"superres_10to{hr}.h5")
    synth = importlib.import_module("sr-for-cfd_amd.synth")
    srcfd.SRModel.from_weights(enc_weights, synth.synthetic_decoder_weights(1), device=-1).save_superres_h5(base)
    m = srcfd.SRModel.from_weights(enc_weights, fam.synthetic_decoder_weights(hr), device=-1)
    m.save_superres_h5(famh5)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sr-for-cfd_amd", "csrc"), "pack_digest"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "sr-for-cfd_amd", "lib", "pack_digest_asan")
    dump = tmp_path / "dump"
    dump.mkdir()
    out = subprocess.run([exe, base, str(dump), famh5], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    sec = {s["name"]: s for s in json.loads(out.stdout)["sections"]}
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "operand_pack_digests.json")))["sections"]
    assert all((sec[n]["off"], sec[n]["len"], sec[n]["sha256"]) == (g["off"], g["len"], g["sha256"]) for n, g in golden.items())   # existing packs: same bytes
    extra = sorted(set(sec) - set(golden))
    assert extra and all(n.startswith("family.") for n in extra)
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "family_pack_digests.json")))["files"][f"decoder_{hr}"]
    assert extra == sorted(recorded), sorted(set(extra) ^ set(recorded))
    assert any(n.startswith("family.any16.bf16.") for n in extra) and any(n.startswith("family.any16.f16.") for n in extra)
    bad = [n for n, g in recorded.items() if (sec[n]["off"], sec[n]["len"], sec[n]["sha256"]) != (g["off"], g["len"], g["sha256"])]
    assert not bad, f"family sections of decoder_{hr} that differ from the recorded bytes / offsets: {bad}"
    return m, sec, dump


def test_pack_harness_decoder_10_matches_the_recorded_digests(srcfd, enc_weights, tmp_path):
    """The smallest family graph: no narrow-channel op, every GEMM op padded to 64 / 64."""
    m, sec, dump = _family_harness(srcfd, enc_weights, tmp_path, 10)
    assert m.output_shape == (10, 10, 1) and sec["family.any16.bf16.Wt"]["len"] == sec["family.any16.f16.Wt"]["len"] > 0


def test_pack_harness_family_mode_runs_clean(srcfd, enc_weights, tmp_path):
    """tools/pack_digest.cpp with a family file: build_plan and build_dgrad of padding='same' layers under ASan / UBSan, the
    descriptors of the cropped phases, the weight-gradient maps as bijections onto the parameters, and every `family.*` section
    (the 16-bit packs of the graph among them) against its recorded digest."""
    m, sec, dump = _family_harness(srcfd, enc_weights, tmp_path, 80)
    # encoder (4 ops) + dense_1 + four 3x3 stride-2 'same' layers of four phases + the output convolution
    assert sec["family.ops_off"]["len"] == 2 * (4 + 1 + 16 + 1)
    # the 16-bit packs of this graph: built for both operand types; the output convolution's weights are 16-bit values
    lp = importlib.import_module("oracle.sr_oracle_lowp")
    assert sec["family.any16.bf16.Wt"]["len"] == sec["family.any16.f16.Wt"]["len"] > 0 and sec["family.any16.bf16.w_off"]["len"] == 4 * 20
    wout = np.fromfile(str(dump / "family.any16.bf16.wout.bin"), np.float32)
    k = m.weights()["output_image_80/kernel"].reshape(-1)
    assert np.array_equal(wout, lp.round_bf16(np.asarray(k, np.float64) / lp.LOG2E))
    wout = np.fromfile(str(dump / "family.any16.f16.wout.bin"), np.float32)
    assert np.array_equal(wout, lp.round_f16(np.asarray(k, np.float64) / lp.LOG2E))
    ops = np.loadtxt(str(dump / "family.train.ops.txt"), dtype=np.int64)   # K N Npad layer nphx
    n_params = sum(v.size for v in m.weights().values())
    seen = []
    for i, (K, N, Npad, layer, nphx) in enumerate(ops):
        g = np.fromfile(str(dump / f"family.train.op{i}.gmap.bin"), np.int32).reshape(K + 1, Npad)
        assert (g[:, N:] == 0).all() and (g[:, :N] > 0).all()
        seen.append(g[:K, :N].ravel())
        seen.append(g[K, :N])
    allp = np.unique(np.concatenate(seen))
    assert np.array_equal(allp, np.arange(1, n_params + 1))                # every parameter is reached
    w = np.concatenate(seen[0::2])
    assert np.unique(w).size == w.size                                      # and every kernel weight by exactly one slot
