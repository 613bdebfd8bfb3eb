"""The device scorer (csrc/score.hip) on an MI355X against numpy: `score_fields`, `EvalSet.score` and `fit(validation=...)`.
Every comparison is equality of float32 bit patterns, NaNs in the same places -- there is no tolerance in this file.  The
reference is tests/score_ref.py's `notebook_metrics`: the literal numpy expressions of `evaluate_for_re`
(sr-ae-conv.ipynb:c323-369) on the arrays numpy sees, i.e. on `model.predict(x)` of the same handle for the EvalSet tests."""
import importlib

import numpy as np
import pytest

import score_ref as sr
from conftest import require_gpu

pytestmark = pytest.mark.gpu


def _family():
    return importlib.import_module("sr-for-cfd_amd.family")


def _fields(n, elems, seed):
    """Mixed-sign prediction and truth with different spreads, and (mean, std) pairs per sample."""
    rng = np.random.default_rng(seed)
    pred = rng.standard_normal((n, elems)).astype(np.float32)
    truth = (rng.standard_normal((n, elems)) * 1.3 + 0.2).astype(np.float32)
    pa = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(0.05, 2.0, n)], axis=1).astype(np.float32)
    ta = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(0.05, 2.0, n)], axis=1).astype(np.float32)
    return pred, truth, pa, ta


# ---------------------------------------------------------------------------------------------- 1. score_fields
@pytest.mark.parametrize("elems", [e for e in sr.LENGTHS if e <= 16385] + [160_000])
def test_score_fields_has_numpys_bits(srcfd, elems):
    require_gpu(srcfd)
    n = 3
    pred, truth, pa, ta = _fields(n, elems, seed=elems)
    modes = [("both", pa, ta)] if elems == 160_000 else [("both", pa, ta), ("pred", pa, None), ("truth", None, ta), ("none", None, None)]
    for name, a, b in modes:
        got = srcfd.score_fields(pred, truth, pred_affine=a, truth_affine=b)
        assert set(got) == set(sr.NAMES) and all(v.dtype == np.float32 and v.shape == (n,) for v in got.values())
        sr.assert_same_bits(got, sr.notebook_metrics(pred, truth, a, b), f"elems={elems} affines={name}")


def test_score_fields_takes_image_shaped_arrays(srcfd):
    """(n, h, w, 1) arrays, an odd side (no 16-byte rows) and the shared affine of `evaluate_for_re`."""
    require_gpu(srcfd)
    pred, truth, pa, _ = _fields(2, 81 * 81, seed=81)
    pred, truth = pred.reshape(2, 81, 81, 1), truth.reshape(2, 81, 81, 1)
    sr.assert_same_bits(srcfd.score_fields(pred, truth, pa, pa), sr.notebook_metrics(pred, truth, pa, pa), "81x81")


# ---------------------------------------------------------------------------------------------- 2. edge values
@pytest.mark.parametrize("elems", [8193, 129])
def test_edge_values(srcfd, elems):
    require_gpu(srcfd)
    n = 6
    pred, truth, pa, ta = _fields(n, elems, seed=7 + elems)
    pred[0, elems // 3] = np.nan                      # one NaN in pred: MAE, MSE, MAX_ABS and the pred range are NaN
    truth[1, elems - 1] = np.inf                      # one +Inf in truth, in the last (unbalanced) leaf
    pred[2, :] = truth[2, :] = np.float32(0.625)      # a constant field: range 0
    pa, ta = pa.copy(), ta.copy()
    pa[3, 1] = 0.0                                    # std = 0: the prediction collapses to the mean
    ta[4, 1] = 0.0
    pred[5, 0], truth[5, 5], pred[5, elems - 1] = np.nan, np.nan, -np.inf   # several kinds at once
    for name, a, b in (("both", pa, ta), ("none", None, None)):
        want = sr.notebook_metrics(pred, truth, a, b)
        got = srcfd.score_fields(pred, truth, a, b)
        sr.assert_same_bits(got, want, f"elems={elems} affines={name}")
        assert np.isnan(got["mae"][0]) and np.isnan(got["mse"][0]) and np.isnan(got["max_abs"][0])
        assert np.isnan(got["pred_min"][0]) and np.isnan(got["pred_max"][0]) and np.isfinite(got["truth_min"][0])
        assert np.isinf(got["truth_max"][1]) and np.isinf(got["mae"][1]) and np.isfinite(got["pred_max"][1])
        assert got["nonfinite"].tolist()[:3] == [1.0, 1.0, 0.0] and got["nonfinite"][5] == 3.0
        if a is None:
            assert got["truth_min"][2] == got["truth_max"][2] == np.float32(0.625) and got["mae"][2] == 0
        else:
            assert got["pred_min"][3] == got["pred_max"][3] == pa[3, 0]


# ---------------------------------------------------------------------------------------------- 3. sample independence
def test_a_sample_does_not_depend_on_its_batch(srcfd):
    require_gpu(srcfd)
    pred, truth, pa, ta = _fields(5, 10_000, seed=3)
    whole = srcfd.score_fields(pred, truth, pa, ta)
    for i in range(5):
        one = srcfd.score_fields(pred[i:i + 1], truth[i:i + 1], pa[i:i + 1], ta[i:i + 1])
        sr.assert_same_bits({k: v[i:i + 1] for k, v in whole.items()}, one, f"sample {i}")


# ---------------------------------------------------------------------------------------------- 4. - 6. EvalSet
def _model(srcfd, enc_weights, hr, dec_weights=None):
    dec = dec_weights if hr == 400 else _family().synthetic_decoder_weights(hr)
    return srcfd.SRModel.from_weights(enc_weights, dec, device=0)


def _set(n, hr, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 10, 10, 1)).astype(np.float32)
    truth = (rng.standard_normal((n, hr, hr, 1)) * 0.8).astype(np.float32)
    ia = np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(0.5, 1.5, n)], axis=1).astype(np.float32)
    pa = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(0.05, 2.0, n)], axis=1).astype(np.float32)
    return x, truth, ia, pa


def _numpy_on_predict(model, x, truth, ia, pa, ta):
    """numpy on `model.predict(x)`: the standardised prediction of the same handle, same n, same precision, into pageable memory."""
    n = len(x)
    pred = model.predict(x, in_affine=ia, out=np.empty((n,) + model.output_shape, np.float32))
    return sr.notebook_metrics(pred, truth, pa, ta)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("hr,n", [(20, 7), (400, 3)])
def test_evalset_score_equals_numpy_on_predict(srcfd, enc_weights, dec_weights, hr, n, precision):
    require_gpu(srcfd)
    model = _model(srcfd, enc_weights, hr, dec_weights)
    model.precision = precision
    x, truth, ia, pa = _set(n, hr, seed=hr + n)
    es = srcfd.EvalSet(x, truth, in_affine=ia, pred_affine=pa, truth_affine=pa)
    got = es.score(model)
    want = _numpy_on_predict(model, x, truth, ia, pa, pa)
    sr.assert_same_bits(got, want, f"decoder_{hr} n={n} {precision}")
    # train_main.evaluate_for_re's formula on the arrays
    pred = model.predict(x, in_affine=ia, out=np.empty((n, hr, hr, 1), np.float32))
    for i in range(n):
        p = pred[i, ..., 0] * pa[i, 1] + pa[i, 0]
        t = truth[i, ..., 0] * pa[i, 1] + pa[i, 0]
        mae = float(np.mean(np.abs(t - p)))
        assert got["nmae_percent"][i] == mae / (float(np.max(t) - np.min(t)) + 1e-8) * 100, i
    # a second score of the same set (the forward is now replayed from its graph) and a set without affines
    sr.assert_same_bits(es.score(model), want, "second score")
    plain = srcfd.EvalSet(x, truth)
    sr.assert_same_bits(plain.score(model), _numpy_on_predict(model, x, truth, None, None, None), "no affines")
    es.close()
    plain.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_evalset_crosses_the_staging_chunk(srcfd, enc_weights, precision):
    """300 samples = one chunk of 256 (Model::STAGE_SAMPLES) and one of 44."""
    require_gpu(srcfd)
    model = _model(srcfd, enc_weights, 20)
    model.precision = precision
    n = 300
    x, truth, ia, pa = _set(n, 20, seed=300)
    es = srcfd.EvalSet(x, truth, in_affine=ia, pred_affine=pa, truth_affine=pa)
    got = es.score(model)
    want = _numpy_on_predict(model, x, truth, ia, pa, pa)
    for row in (255, 256, 299):
        sr.assert_same_bits({k: got[k][row:row + 1] for k in want}, {k: v[row:row + 1] for k, v in want.items()}, f"row {row} ({precision})")
    sr.assert_same_bits(got, want, f"all 300 rows ({precision})")
    es.close()


def test_scoring_leaves_the_model_as_it_was(srcfd, enc_weights):
    require_gpu(srcfd)
    model = _model(srcfd, enc_weights, 20)
    model.precision = "bf16"
    x, truth, ia, pa = _set(5, 20, seed=11)
    before = model.predict(x, in_affine=ia).copy()
    es = srcfd.EvalSet(x[:3], truth[:3], in_affine=ia[:3], pred_affine=pa[:3], truth_affine=pa[:3])
    es.score(model)
    assert model.precision == "bf16" and model.last_plan()["precision"] == "bf16"
    after = model.predict(x, in_affine=ia)
    np.testing.assert_array_equal(before.view(np.uint32), after.view(np.uint32))
    assert model.last_plan()["precision"] == "bf16"
    es.close()


# ---------------------------------------------------------------------------------------------- 7. fit(validation=...)
def test_fit_with_validation(srcfd):
    """Validation after each of two epochs equals a score of the weights a separate, identical run has at that epoch, and
    changes nothing of the training: losses and final weights are those of a run without validation."""
    require_gpu(srcfd)
    tr = importlib.import_module("sr-for-cfd_amd.train")
    rng = np.random.default_rng(21)
    xl = rng.standard_normal((6, 10, 10, 1)).astype(np.float32)
    xh = rng.standard_normal((6, 20, 20, 1)).astype(np.float32)
    vx, vt, _, pa = _set(4, 20, seed=22)

    def run(epochs, validation=None, every=1):
        enc, dec = _family().keras_default_init(10, 20, 5)
        t = tr.Trainer(srcfd.SRModel.from_weights(enc, dec, device=0, lr_dim=10, hr_dim=20), max_batch=4)
        hist = tr.fit(t, xl, xh, epochs=epochs, batch_size=4, seed=1, validation=validation, validation_every=every)
        return t, hist

    es = srcfd.EvalSet(vx, vt, pred_affine=pa, truth_affine=pa)
    t_val, hist_val = run(2, es)
    assert [e["epoch"] for e in es.history] == [1, 2]
    fresh = srcfd.EvalSet(vx, vt, pred_affine=pa, truth_affine=pa)
    # the separate runs: one epoch (with a set that is due every 5th epoch: scored after the last one only), two epochs without validation
    late = srcfd.EvalSet(vx, vt, pred_affine=pa, truth_affine=pa)
    stopped = {1: run(1, late, every=5), 2: run(2)}
    assert [e["epoch"] for e in late.history] == [1]
    for epochs, (t_plain, _) in stopped.items():
        model = t_plain.export_model()
        want = fresh.score(model)
        model.close()
        entry = es.history[epochs - 1]
        sr.assert_same_bits(entry["per_sample"], want, f"epoch {epochs}")
        np.testing.assert_array_equal(entry["per_sample"]["nmae_percent"], want["nmae_percent"])
        assert entry["val_mae"] == float(np.mean(want["mae"], dtype=np.float64))
        assert entry["val_mse"] == float(np.mean(want["mse"], dtype=np.float64))
        assert entry["val_nmae_percent"] == float(np.mean(want["nmae_percent"], dtype=np.float64))
    sr.assert_same_bits(late.history[0]["per_sample"], es.history[0]["per_sample"], "epoch 1, scored as the last epoch")
    t_plain, hist_plain = stopped[2]
    assert hist_val == hist_plain and len(hist_val) == 2 and hist_val[:1] == stopped[1][1]
    w_val, w_plain = t_val.weights(), t_plain.weights()
    for k in w_plain:
        np.testing.assert_array_equal(w_val[k].view(np.uint32), w_plain[k].view(np.uint32), err_msg=k)
    for s_ in (es, fresh, late):
        s_.close()


def test_training_driver_reports_validation(srcfd, tmp_path, capsys):
    """`train_main.py --validate-every 2` on a three-epoch run of the 10 -> 20 member: the report gains a "validation" list with
    epochs 2 and 3 (every second epoch, and the last), the existing keys stay, and the last entry is the held-out set scored with the
    weights `evaluate_for_re` reports on.  Those two differ in how many samples a forward takes (3 against 1), which may choose
    other f32 kernels, so that one comparison is to f32 rounding of the prediction (1e-4 relative), not to the bit."""
    require_gpu(srcfd)
    import json
    ds = importlib.import_module("sr-for-cfd_amd.datasets")
    h5 = importlib.import_module("sr-for-cfd_amd.h5")
    main = importlib.import_module("sr-for-cfd_amd.train_main")
    rng = np.random.default_rng(5)
    w = h5.H5Writer()
    for Re in (100, 200, 800):
        base = {c: rng.standard_normal((20, 20)) for c in "uvp"}
        ds.append_solution(w, Re, 20, base, "single_lid(u_top=1)")
        ds.append_solution(w, Re, 10, {c: ds.avg_pool(base[c][None, ..., None].astype(np.float32), 2)[0, ..., 0] for c in "uvp"}, "single_lid(u_top=1)")
    data = str(tmp_path / "simulation_result.h5")
    w.save(data)
    args = ["--data", data, "--hr-dim", "20", "--epochs", "3", "--suffix", "t", "--out-dir", str(tmp_path), "--log-every", "0"]
    main.main(args + ["--validate-every", "2"])
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert [e["epoch"] for e in rep["validation"]] == [2, 3]
    assert all(set(e) == {"epoch", "val_mae", "val_nmae_percent", "val_mse"} and all(np.isfinite(list(e.values()))) for e in rep["validation"])
    assert rep["train_samples"] == 6 and len(rep["Re800"]["mae"]) == 3
    assert np.isclose(rep["validation"][-1]["val_mae"], rep["average_mae"], rtol=1e-4, atol=0)
    assert np.isclose(rep["validation"][-1]["val_nmae_percent"], rep["average_nmae_percent"], rtol=1e-4, atol=0)
    main.main(args)                                        # the default: today's report
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "validation" not in plain and plain["average_mae"] == rep["average_mae"] and plain["final_recon_loss"] == rep["final_recon_loss"]


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(srcfd, enc_weights):
    require_gpu(srcfd)
    model = _model(srcfd, enc_weights, 20)
    x, truth, ia, pa = _set(2, 50, seed=50)
    other = srcfd.EvalSet(x, truth)                       # 10x10 -> 50x50 set, 10x10 -> 20x20 model
    with pytest.raises(ValueError, match="2500"):
        other.score(model)
    other.close()
    with pytest.raises(ValueError, match="closed"):       # an error, not a crash
        other.score(model)
    other.close()                                          # closing twice is harmless
    empty = srcfd.EvalSet(np.zeros((0, 10, 10, 1), np.float32), np.zeros((0, 20, 20, 1), np.float32))
    got = empty.score(model)
    assert set(got) == set(sr.NAMES) | {"nmae_percent"} and all(len(v) == 0 for v in got.values())
    got = srcfd.score_fields(np.zeros((0, 400), np.float32), np.zeros((0, 400), np.float32))
    assert all(v.shape == (0,) for v in got.values())
    with pytest.raises(ValueError):
        srcfd.score_fields(np.zeros((2, 400), np.float32), np.zeros((2, 401), np.float32))
    with pytest.raises(ValueError, match="2560000"):
        srcfd.score_fields(np.zeros((1, 2_560_001), np.float32), np.zeros((1, 2_560_001), np.float32))
    with pytest.raises(ValueError):
        srcfd.score_fields(np.zeros((2, 400), np.float32), np.zeros((2, 400), np.float32), pred_affine=np.zeros((3, 2), np.float32))
    host = srcfd.SRModel.from_weights(enc_weights, _family().synthetic_decoder_weights(20), device=-1)
    ok = srcfd.EvalSet(x, np.zeros((2, 20, 20, 1), np.float32))
    with pytest.raises(srcfd.NoDeviceError):
        ok.score(host)
    ok.close()
