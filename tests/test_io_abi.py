"""CPU tests of the file formats and the C-ABI surface (no compute calls)."""
import ctypes
import hashlib
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ENCODER_H5, GOLDEN, ROOT, STATS_TXT

# What foreign HDF5 readers (h5py, h5dump) returned on the files these tests write, recorded once by
# tests/golden/record_foreign_readers.py: the writer is deterministic, so a file whose bytes match the record is the file they read.
def _foreign(key):
    with open(os.path.join(GOLDEN, "foreign_readers.json")) as f:
        return json.load(f)[key]


def _sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def write_round_trip_file(srcfd, path):
    """The small file of test_writer_round_trip_and_foreign_readers; returns the arrays written."""
    rng = np.random.default_rng(0)
    w = srcfd.H5Writer()
    a = rng.standard_normal((3, 3, 8, 1)).astype(np.float32)
    b = rng.standard_normal(100)
    c = np.arange(12, dtype=np.int64).reshape(3, 4)
    w.dataset("model_weights/x/x/kernel", a)
    w.dataset("Re400_mesh10x10/u", b)
    w.dataset("ints", c)
    for i in range(40):  # > one symbol-table node
        w.dataset(f"many/d{i:02d}", np.full(3, i, np.float32))
    w.attr("/", "backend", "tensorflow", utf8=True)
    w.attr("/model_weights", "layer_names", ["x", "a_much_longer_layer_name", ""])
    w.attr("/model_weights/x", "weight_names", [])
    w.attr("/Re400_mesh10x10", "lx", 10.0)
    w.attr("/Re400_mesh10x10", "nx", 10)
    w.attr("/", "big", "J" * 20000)
    w.save(path)
    return a, b, c


# ---------------------------------------------------------------- C ABI ------
def _declared_functions():
    text = open(os.path.join(ROOT, "include", "srcfd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(srcfd_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound(srcfd):
    from importlib import import_module
    L = import_module("sr-for-cfd_amd._lib")
    names = _declared_functions()
    assert len(names) >= 35
    lib = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/srcfd.h but not exported"
    assert set(names) == set(L.EXPORTED), set(names) ^ set(L.EXPORTED)
    # the read-only record of the last training step: six pointers (the handle and five ints), and no stream among them
    assert "srcfd_trainer_last_step" in names and len(L.lib.srcfd_trainer_last_step.argtypes) == 6
    assert L.lib.srcfd_trainer_last_step(None, None, None, None, None, None) < 0   # a null handle is a status, and needs no device


def test_library_is_in_tree_and_links_hip(srcfd):
    assert srcfd.LIB_PATH.startswith(ROOT)
    out = subprocess.check_output(["ldd", srcfd.LIB_PATH], text=True)
    assert "libamdhip64" in out


def test_compute_fails_loudly_without_device(srcfd, enc_weights):
    if srcfd.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(srcfd.NoDeviceError):
        srcfd.SRModel.load_h5(ENCODER_H5, None, device=0)
    m = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1)
    with pytest.raises(srcfd.NoDeviceError):
        m.predict(np.zeros((1, 10, 10, 1), np.float32))
    with pytest.raises(srcfd.NoDeviceError):
        m.reserve(4)                     # set-up of device workspaces needs a device, too
    with pytest.raises(ValueError):
        m.reserve(-1)


def test_precision_switch_rules(srcfd, enc_weights, dec_weights):
    m = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1)
    assert not m.has_fused_path
    with pytest.raises(ValueError):
        m.precision = "bf16"  # encoder alone is not the fused graph
    m.precision = "fp32_naive"
    assert m.precision == "fp32_naive"
    full = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=-1)
    full.precision = "bf16"
    assert full.precision == "bf16"


# ---------------------------------------------------------------- HDF5 -------
def test_encoder_h5_structure_and_values(srcfd):
    with srcfd.H5File(ENCODER_H5) as f:
        assert f.attr_str("/", "keras_version") == ["3.8.0"]
        assert f.attr_str("/", "backend") == ["tensorflow"]
        assert f.attr_str("/model_weights", "layer_names") == ["encoder_10_input", "conv2d", "conv2d_1", "flatten", "dense", "latent_vector"]
        assert f.attr_str("/model_weights/conv2d", "weight_names") == ["conv2d/kernel", "conv2d/bias"]
        assert f.attr_str("/model_weights/flatten", "weight_names") == []
        assert sorted(f.keys("/model_weights")) == sorted(["conv2d", "conv2d_1", "dense", "encoder_10_input", "flatten", "latent_vector", "top_level_model_weights"])
        assert f.shape_dtype("/model_weights/conv2d_1/conv2d_1/kernel") == ((3, 3, 64, 128), np.float32)
        k = f["/model_weights/dense/dense/kernel"]
        assert k.shape == (3200, 128) and k.dtype == np.float32 and np.isfinite(k).all() and k.std() > 0
        assert "/model_weights/nope" not in f
        with pytest.raises(KeyError):
            f.read("/model_weights/nope/x")
        cfg = f.attr_str("/", "model_config")[0]
        assert '"class_name": "Functional"' in cfg and '"activation": "silu"' in cfg


def test_reader_agrees_with_h5py(srcfd):
    # h5py's read of the same dataset, stored by tests/golden/record_foreign_readers.py
    assert _sha256(ENCODER_H5) == _foreign("encoder_h5_sha256")
    with srcfd.H5File(ENCODER_H5) as f:
        np.testing.assert_array_equal(f["/model_weights/conv2d_1/conv2d_1/kernel"], np.load(os.path.join(GOLDEN, "h5py_conv2d_1_kernel.npy")))


def test_model_loader_parses_config_and_weights(srcfd):
    m = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1)
    L = m.layers()
    assert [l["name"] for l in L] == ["conv2d", "conv2d_1", "flatten", "dense", "latent_vector"]
    assert (L[0]["stride"], L[0]["same"], L[0]["activation"]) == (2, True, 1)  # swish serialised as "silu"
    assert (L[1]["stride"], L[1]["cin"], L[1]["cout"]) == (1, 64, 128)
    assert L[4]["activation"] == 0 and L[4]["cout"] == 50
    with srcfd.H5File(ENCODER_H5) as f:
        np.testing.assert_array_equal(L[3]["kernel"], f["/model_weights/dense/dense/kernel"])
        np.testing.assert_array_equal(L[0]["bias"], f["/model_weights/conv2d/conv2d/bias"])


def test_model_errors_follow_reference_conventions(srcfd, tmp_path):
    with pytest.raises(FileNotFoundError):  # PyCFD_ML_accelerated.py:1080-1087
        srcfd.SRModel.load_h5(str(tmp_path / "missing.h5"), None, device=-1)
    bad = tmp_path / "bad.h5"
    bad.write_bytes(b"not an hdf5 file" * 20)
    with pytest.raises(OSError):  # PyCFD_ML_accelerated.py:835-837
        srcfd.SRModel.load_h5(str(bad), None, device=-1)
    trunc = tmp_path / "trunc.h5"
    trunc.write_bytes(open(ENCODER_H5, "rb").read()[:200000])
    with pytest.raises(OSError):
        srcfd.SRModel.load_h5(str(trunc), None, device=-1)
    # decoder half chained onto a mismatching encoder
    with pytest.raises(OSError):
        srcfd.SRModel.load_h5(ENCODER_H5, ENCODER_H5, device=-1)


def test_writer_round_trip_and_foreign_readers(srcfd, tmp_path):
    p = tmp_path / "rt.h5"
    a, b, c = write_round_trip_file(srcfd, p)
    with srcfd.H5File(p) as f:
        np.testing.assert_array_equal(f["model_weights/x/x/kernel"], a)
        np.testing.assert_array_equal(f["Re400_mesh10x10/u"], b)
        np.testing.assert_array_equal(f["ints"], c)
        assert f.read("Re400_mesh10x10/u", np.float32).dtype == np.float32
        assert len(f.keys("many")) == 40 and f["many/d39"][0] == 39
        assert f.attr_str("/", "backend") == ["tensorflow"]
        assert f.attr_str("/model_weights", "layer_names") == ["x", "a_much_longer_layer_name", ""]
        assert f.attr_str("/model_weights/x", "weight_names") == []
        assert f.attr_num("/Re400_mesh10x10", "lx")[0] == 10.0 and f.attr_num("/Re400_mesh10x10", "nx")[0] == 10
        assert f.attr_str("/", "big")[0] == "J" * 20000
    rec = _foreign("round_trip")
    assert _sha256(p) == rec["sha256"]          # the very file h5dump and h5py read
    assert "17, 17, 17" in rec["h5dump_many_d17"]
    h = rec["h5py"]
    assert h["backend"] == "tensorflow" and h["layer_names"] == ["x", "a_much_longer_layer_name", ""]
    assert h["ints_2_3"] == 11 and h["many_len"] == 40 and h["nx"] == [10]


def test_keras_h5_save_load_round_trip(srcfd, oracle, enc_weights, dec_weights, tmp_path):
    """srcfd_model_save_h5 writes the legacy layout `encoder.save(...)` produces
    (sr-ae-conv.ipynb:c584-585); loading it back yields identical tensors, and the
    synthetic decoder file exercises the decoder half of the loader."""
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=-1)
    e, d = tmp_path / "enc.h5", tmp_path / "dec.h5"
    # from_weights builds one sub-model; save it, then split through two loads
    srcfd.SRModel.from_weights(enc_weights, None, device=-1).save_h5(str(e))
    srcfd.SRModel.from_weights(None, dec_weights, device=-1).save_h5(None, str(d))
    m2 = srcfd.SRModel.load_h5(str(e), str(d), device=-1)
    assert m2.has_fused_path and m2.macs_per_sample == m.macs_per_sample
    w1, w2 = m.weights(), m2.weights()
    assert list(w1) == list(w2) and len(w1) == 22
    for k in w1:
        np.testing.assert_array_equal(w1[k], w2[k])
        np.testing.assert_array_equal(w1[k], {**enc_weights, **dec_weights}[k])
    with srcfd.H5File(d) as f:
        assert f.attr_str("/", "keras_version") == ["3.8.0"]
        names = f.attr_str("/model_weights", "layer_names")
        assert names == ["model_input", "dense_1", "reshape", "conv2d_transpose", "conv2d_transpose_1", "conv2d_transpose_2",
                         "conv2d_transpose_3", "conv2d_transpose_4", "output_image_400"]
    rec = _foreign("decoder")
    assert _sha256(d) == rec["sha256"]          # the very file h5py read
    assert rec["h5py"]["class_name"] == "Functional" and rec["h5py"]["layers"] == 9 and rec["h5py"]["convT0_kernel_shape"] == [3, 3, 128, 256]


def test_whole_model_superres_file_round_trip(srcfd, enc_weights, dec_weights, tmp_path):
    """`superres_model.save("superres_10to400_vanilla_ae_*.h5")` (sr-ae-conv.ipynb:c586): encoder + decoder in one legacy
    Keras-H5 file, groups model_weights/<sub-model>/<layer>/{kernel,bias} (the layout is unpinned: the reference's files are
    absent).  Round trip through the nested sub-model configs, and through the fallback that assumes the reference
    architecture when a file has weights only."""
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=-1)
    p = str(tmp_path / "superres_10to400_vanilla_ae_test.h5")
    m.save_superres_h5(p)
    m2 = srcfd.SRModel.load_superres_h5(p, device=-1)
    assert m2.has_fused_path and m2.input_shape == (10, 10, 1) and m2.output_shape == (400, 400, 1)
    assert m2.macs_per_sample == m.macs_per_sample == 140_024_128
    w1, w2 = m.weights(), m2.weights()
    assert list(w1) == list(w2) and len(w1) == 22
    for k in w1:
        np.testing.assert_array_equal(w1[k], w2[k])
    assert [(d["name"], d["stride"], d["same"], d["activation"]) for d in m2.layers()] == \
           [(d["name"], d["stride"], d["same"], d["activation"]) for d in m.layers()]
    with srcfd.H5File(p) as f:
        assert f.attr_str("/model_weights", "layer_names") == ["encoder_10", "decoder_400"]
        assert f.attr_str("/model_weights/encoder_10", "weight_names")[:2] == ["conv2d/kernel", "conv2d/bias"]
        assert f.shape_dtype("/model_weights/decoder_400/conv2d_transpose/kernel")[0] == (3, 3, 128, 256)
        assert "SuperResolutionAE" in f.attr_str("/", "model_config")[0]
    # a weights-only variant (no sub-model configs in model_config): the reader falls back to the reference architecture
    w = srcfd.H5Writer()
    w.attr("/", "keras_version", "3.8.0")
    w.attr("/", "backend", "tensorflow")
    w.attr("/", "model_config", '{"class_name": "SuperResolutionAE"}')
    w.group("model_weights")
    w.attr("/model_weights", "layer_names", ["encoder_10", "decoder_400"])
    for sub, ws in (("encoder_10", enc_weights), ("decoder_400", dec_weights)):
        w.group(f"model_weights/{sub}")
        w.attr(f"/model_weights/{sub}", "weight_names", list(ws))
        for k, v in ws.items():
            w.dataset(f"model_weights/{sub}/{k}", v)
    q = str(tmp_path / "superres_weights_only.h5")
    w.save(q)
    m3 = srcfd.SRModel.load_superres_h5(q, device=-1)
    assert m3.has_fused_path and [(d["name"], d["stride"], d["same"], d["activation"], d["reshape"]) for d in m3.layers()] == \
                                  [(d["name"], d["stride"], d["same"], d["activation"], d["reshape"]) for d in m.layers()]
    for k in w1:
        np.testing.assert_array_equal(m3.weights()[k], w1[k])
    # ... and ONLY for that architecture: the notebook's other variants carry the same layer names with other strides /
    # paddings, which a weights-only file cannot express -- a 3x3 transposed kernel where the reference has 2x2 is refused
    def weights_only(path, enc_w, dec_w):
        ww = srcfd.H5Writer()
        ww.attr("/", "keras_version", "3.8.0")
        ww.attr("/", "backend", "tensorflow")
        ww.attr("/", "model_config", '{"class_name": "SuperResolutionAE"}')
        ww.group("model_weights")
        ww.attr("/model_weights", "layer_names", ["encoder_10", "decoder_400"])
        for sub, ws in (("encoder_10", enc_w), ("decoder_400", dec_w)):
            ww.group(f"model_weights/{sub}")
            ww.attr(f"/model_weights/{sub}", "weight_names", list(ws))
            for k, v in ws.items():
                ww.dataset(f"model_weights/{sub}/{k}", v)
        ww.save(path)
    other = dict(dec_weights)
    k1 = dec_weights["conv2d_transpose_1/kernel"]
    other["conv2d_transpose_1/kernel"] = np.zeros((3, 3) + k1.shape[2:], np.float32)      # Conv2DTranspose(.., 3, strides=2, padding='same') variant
    bad = str(tmp_path / "superres_other_variant.h5")
    weights_only(bad, enc_weights, other)
    with pytest.raises(OSError, match="architecture not recoverable"):
        srcfd.SRModel.load_superres_h5(bad, device=-1)
    fewer = {k: v for k, v in dec_weights.items() if not k.startswith("conv2d_transpose_4/")}
    weights_only(bad, enc_weights, fewer)
    with pytest.raises(OSError, match="architecture not recoverable"):
        srcfd.SRModel.load_superres_h5(bad, device=-1)
    # the sub-model pair written from it is what the solvers load (PyCFD_ML_accelerated.py:831-832)
    m3.save_h5(str(tmp_path / "e.h5"), str(tmp_path / "d.h5"))
    assert srcfd.SRModel.load_h5(str(tmp_path / "e.h5"), str(tmp_path / "d.h5"), device=-1).macs_per_sample == 140_024_128
    # errors: a sub-model file is not a whole-model file; missing file
    with pytest.raises(OSError):
        srcfd.SRModel.load_superres_h5(ENCODER_H5, device=-1)
    with pytest.raises(FileNotFoundError):
        srcfd.SRModel.load_superres_h5(str(tmp_path / "nope.h5"), device=-1)
    rec = _foreign("superres")
    assert _sha256(p) == rec["sha256"]          # the very file h5py read
    assert rec["h5py"]["class_name"] == "SuperResolutionAE" and rec["h5py"]["first_config_key"] == "decoder_hr"
    assert rec["h5py"]["dense_1_kernel_shape"] == [50, 36864]


# ---------------------------------------------------------------- stats ------
def test_stats_parser_matches_reference_rules(srcfd, oracle, tmp_path):
    lr, hr = srcfd.load_stats(STATS_TXT, 10, 400)
    o_lr, o_hr = oracle.component_stats(oracle.parse_stats(STATS_TXT), 10, 400)
    assert lr == o_lr and hr == o_hr
    assert lr["u"] == (0.0001939494695193795, 0.23378464769154605)
    p = tmp_path / "s.txt"
    p.write_text("# comment\n\n   # indented comment\nmean10_u 1.5\nstd10_u 2\nthree tokens here\nlonely\n"
                 "mean10_v 0\nstd10_v 1\nmean10_p -1e-3\nstd10_p 1\nmean400_u 0\nstd400_u 1\nmean400_v 0\nstd400_v 1\n"
                 "mean400_p 0\nstd400_p 1\nmean10_u 2.5\n")
    lr, _ = srcfd.load_stats(p, 10, 400)
    assert lr["u"] == (2.5, 2.0) and lr["p"][0] == -1e-3  # later duplicates win, like a dict
    with pytest.raises(KeyError):
        srcfd.load_stats(p, 10, 100)
    with pytest.raises(FileNotFoundError):
        srcfd.load_stats(tmp_path / "nope.txt", 10, 400)
    q = tmp_path / "w.txt"
    srcfd.save_stats(q, 10, 400, o_lr, o_hr)
    assert srcfd.load_stats(q, 10, 400) == (o_lr, o_hr)
    assert oracle.component_stats(oracle.parse_stats(q), 10, 400) == (o_lr, o_hr)


def test_all_three_reference_stats_files_parse(srcfd):
    for fn in os.listdir(GOLDEN):
        if fn.startswith("standardization_stats"):
            lr, hr = srcfd.load_stats(os.path.join(GOLDEN, fn), 10, 400)
            assert all(s > 0 for _, s in list(lr.values()) + list(hr.values()))


def test_coarse_field_files(srcfd, coarse_cases):
    assert set(coarse_cases) == {"bfs_Re400", "ldc_Re800_single", "ldc_Re1000_single", "ldc_Re800_double", "ldc_Re1000_double"}
    for case in coarse_cases.values():
        for c in ("u", "v", "p"):
            assert case[c].shape == (10, 10) and case[c].dtype == np.float64 and np.isfinite(case[c]).all()
    v = coarse_cases["ldc_Re800_double"]["v"]
    assert abs(v.max() + v.min()) < 1e-6  # double-lid symmetry noted in SURVEY.md section 4


def _mutation_corpus(tmp_path, n_random=120):
    """Structure-aware mutations of the real encoder .h5: random bytes / all-ones / huge 8-byte values near every B-tree,
    symbol-table, heap and superblock signature, truncations, and targeted ones for the parser's size arithmetic:
    dataspace dimensions whose product (or product x element size) wraps 64 bits, contiguous layouts flipped to compact
    or given an undefined address, link names with their terminator removed up to the end of the file, and global-heap
    object sizes that stall or overrun the heap walk."""
    import re
    data = bytearray(open(ENCODER_H5, "rb").read())
    n = len(data)
    sigs = [m.start() for m in re.finditer(b"TREE|SNOD|HEAP|GCOL|\x89HDF", bytes(data))]
    rng = np.random.default_rng(99)
    out = []

    def emit(d, tag):
        p = tmp_path / f"m{len(out)}_{tag}.h5"
        p.write_bytes(bytes(d))
        out.append(str(p))

    for it in range(n_random):
        d = bytearray(data)
        for _ in range(int(rng.integers(1, 5))):
            pos = min(n - 9, int(sigs[int(rng.integers(0, len(sigs)))]) + int(rng.integers(0, 256)))
            mode = rng.random()
            if mode < 0.5:
                d[pos] = int(rng.integers(0, 256))
            elif mode < 0.7:
                d[pos] = 0xFF
            else:
                d[pos:pos + 8] = [2**64 - 1, 2**63 - 1, n + 12345, 1 << 40][int(rng.integers(0, 4))].to_bytes(8, "little")
        if rng.random() < 0.1:
            d = d[: int(rng.integers(100, n))]
        emit(d, "rand")
    # dataspace messages (version 1: 01 rank flags 00 00 00 00 00, then rank x 8-byte dims) of the weight datasets
    spaces = [m.start() for m in re.finditer(b"\x01[\x01-\x04]\x00\x00\x00\x00\x00\x00", bytes(data))]
    wraps = [(1 << 62) + 1, (1 << 63) + 3, (1 << 64) - 1, 1 << 61, (1 << 32) + 1]
    for pos in spaces[:40]:
        rank = data[pos + 1]
        for w in wraps[:3]:
            d = bytearray(data)
            d[pos + 8:pos + 16] = w.to_bytes(8, "little")
            if rank > 1:
                d[pos + 16:pos + 24] = wraps[3].to_bytes(8, "little")
            emit(d, "dims")
    # layout messages, version 3 class 1 (contiguous): 03 01 <addr 8> <size 8>
    layouts = [m.start() for m in re.finditer(b"\x03\x01", bytes(data)) if m.start() + 18 < n and
               int.from_bytes(data[m.start() + 2:m.start() + 10], "little") < n and
               0 < int.from_bytes(data[m.start() + 10:m.start() + 18], "little") < n]
    for pos in layouts[:30]:
        d = bytearray(data); d[pos + 1] = 0; d[pos + 2:pos + 4] = (4).to_bytes(2, "little"); emit(d, "compact")   # 4 bytes of compact data
        d = bytearray(data); d[pos + 2:pos + 10] = b"\xff" * 8; emit(d, "undef_addr")                              # no storage at all
    # names in local heaps: no terminator between a name and the end of the (truncated) file
    for pos in [m.start() for m in re.finditer(b"HEAP", bytes(data))][:10]:
        seg = int.from_bytes(data[pos + 24:pos + 32], "little")                # data segment address
        if 0 < seg < n - 64:
            d = bytearray(data[:min(n, seg + 48)])
            for i in range(seg, len(d)):
                if d[i] == 0:
                    d[i] = 0x41
            emit(d, "name")
    # global heap collections: object sizes of ~2^64 (the padded step wraps to 0: no forward progress) and past the collection
    for pos in [m.start() for m in re.finditer(b"GCOL", bytes(data))][:6]:
        for val in ((1 << 64) - 8, (1 << 64) - 24, 1 << 40):
            d = bytearray(data); d[pos + 24:pos + 32] = val.to_bytes(8, "little"); emit(d, "gheap")      # first object's size
        d = bytearray(data); d[pos + 8:pos + 16] = ((1 << 64) - 1).to_bytes(8, "little"); emit(d, "gcol_size")
    return out


def test_corrupted_weight_files_raise_and_never_crash(tmp_path):
    """The loader must answer every mutated file with an exception (OSError / ValueError / KeyError ...) or load it, never
    crash or hang.  Runs in a child process so that a crash would be a test failure rather than the end of the session."""
    import subprocess
    import sys
    paths = _mutation_corpus(tmp_path)
    code = (
        "import sys, importlib\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "srcfd = importlib.import_module('sr-for-cfd_amd')\n"
        "ok = bad = 0\n"
        "for p in sys.argv[1:]:\n"
        "    try:\n"
        "        m = srcfd.SRModel.load_h5(p, None, device=-1); m.weights(); ok += 1\n"
        "    except Exception:\n"
        "        bad += 1\n"
        "    try:\n"
        "        f = srcfd.H5File(p)\n"
        "        for name in ('model_weights/dense/dense/kernel', 'model_weights/conv2d/conv2d/bias'):\n"
        "            f.read(name)\n"
        "    except Exception:\n"
        "        pass\n"
        "print(ok, bad)\n")
    out = subprocess.run([sys.executable, "-c", code] + paths, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ok, bad = map(int, out.stdout.split())
    assert ok + bad == len(paths) and bad > 0


def test_corrupted_weight_files_under_address_sanitizer(tmp_path):
    """The same corpus through the host-only AddressSanitizer + UBSan build of h5lite.cpp / model.cpp / capi_io.cpp
    (`make -C sr-for-cfd_amd/csrc asan`, harness tools/h5_check.cpp): a silent over-read that an ordinary build survives
    ends this process with a sanitizer report (sanitizers run on the CPU build only)."""
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    csrc = os.path.join(ROOT, "sr-for-cfd_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "sr-for-cfd_amd", "lib", "h5_check_asan")
    clean = subprocess.run([exe, ENCODER_H5], capture_output=True, text=True, timeout=120)
    assert clean.returncode == 0 and clean.stdout.split()[:2] == ["1", "0"], clean.stderr[-2000:]
    paths = _mutation_corpus(tmp_path, n_random=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:allocator_may_return_null=1", UBSAN_OPTIONS="print_stacktrace=1")
    for lo in range(0, len(paths), 100):
        out = subprocess.run([exe] + paths[lo:lo + 100], capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        ok, bad, _ = map(int, out.stdout.split())
        assert ok + bad == len(paths[lo:lo + 100])


def test_every_int_entry_point_runs_inside_the_abi_guard():
    """`never throws across the ABI` (include/srcfd.h; SURVEY.md 8b errors) is enforced structurally: every multi-line
    int-returning extern "C" definition in csrc/ opens with srcfd::abi_guard (resample.hip and most of
    train.hip had new / std::vector with no try / catch)."""
    import re
    src = os.path.join(ROOT, "sr-for-cfd_amd", "csrc")
    seen = 0
    for f in sorted(os.listdir(src)):
        if not f.endswith((".hip", ".cpp")):
            continue
        text = open(os.path.join(src, f)).read()
        for m in re.finditer(r'^(?:extern "C" )?int (srcfd_\w+)\([^;{]*\) \{\n(.*)\n', text, re.M):
            seen += 1
            assert "abi_guard(\"" + m.group(1) + "\"" in m.group(2), (f, m.group(1), m.group(2))
    assert seen >= 40, seen


@pytest.mark.gpu
def test_allocation_failure_is_a_status_not_a_crash(srcfd):
    """An absurd resampling matrix (2^30 x 2^30 doubles) cannot be allocated: std::bad_alloc / length_error inside
    srcfd_resampler_create must come back as a negative status with a message, through the ABI guard."""
    import ctypes as C
    from conftest import require_gpu
    require_gpu(srcfd)
    L = importlib.import_module("sr-for-cfd_amd._lib")
    dummy = np.zeros(8, np.float64)
    h = C.c_void_p()
    rc = L.lib.srcfd_resampler_create(0, dummy.ctypes.data_as(C.c_void_p), dummy.ctypes.data_as(C.c_void_p), 1, 1 << 30, 1, 1 << 30, C.byref(h))
    assert rc in (L.ENOMEM, L.EINVAL) and not h.value, rc
    msg = L.lib.srcfd_last_error().decode()
    assert "srcfd_resampler_create" in msg, msg
    # the library is still usable afterwards: a sane resampler comes up
    eye = np.eye(4)
    rc = L.lib.srcfd_resampler_create(0, eye.ctypes.data_as(C.c_void_p), eye.ctypes.data_as(C.c_void_p), 4, 4, 4, 4, C.byref(h))
    assert rc == 0 and h.value
    L.lib.srcfd_resampler_destroy(h)
