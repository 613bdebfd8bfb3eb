"""bench.py's own surface: a plain run is the headline only, `--full` adds the other measurements, and `--dump-outputs DIR`
writes what the timed path returned in its last timed step."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ENCODER_H5, ROOT, STATS_TXT

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY_KEYS = ("roofline", "kernels_ms", "cpu_baseline", "parity_path", "parity_path_x3", "train", "tiled", "host_io")


def _bench(argv, env_extra=None, timeout=600):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    return p.returncode, [json.loads(ln) for ln in lines], p.stderr


def test_full_is_off_by_default_and_dump_takes_a_directory():
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    idx = bench.dump_index(768)
    assert len(idx) == bench.DUMP_SAMPLES and np.array_equal(idx, bench.dump_index(768))
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 768
    assert np.array_equal(bench.dump_index(48), np.arange(48))
    assert bench.DUMP_SAMPLES * 400 * 400 * 4 <= 64 * 2**20             # the f32 dump of one headline step fits 64 MB
    bench.write_outputs(str(tmp_path / "d"), {"y": np.ones((2, 3), np.float32), "i": np.arange(2, dtype=np.float64)})
    assert np.load(tmp_path / "d" / "y.npy").dtype == np.float32 and np.load(tmp_path / "d" / "i.npy").dtype == np.float64
    with pytest.raises(TypeError):
        bench.write_outputs(str(tmp_path / "d"), {"bad": np.arange(2)})
    # the inputs are a function of the arguments and the rank alone
    lr = {c: (0.1, 2.0) for c in "uvp"}
    for a, b in zip(bench.build_inputs(4, 0, lr, lr), bench.build_inputs(4, 0, lr, lr)):
        assert np.array_equal(a, b)


def test_plain_dry_run_has_no_rank0_legs():
    """The rank rehearsal mirrors a real run: rank 0's CPU leg belongs to --full only."""
    rc, recs, err = _bench(["--gpus", "2", "--steps", "3", "--warmup", "1"], {"SRCFD_BENCH_DRYRUN": "1"})
    assert rc == 0, err[-2000:]
    assert len(recs) == 1 and recs[0]["cpu_baseline"] is None


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_its_last_step(srcfd, tmp_path):
    """A plain run carries the headline keys and none of --full's records; the dumped results are the same in two runs and
    are the network's answer for bench.py's inputs (bf16 tolerance of SURVEY.md 8c against the float64 torch oracle)."""
    import torch
    from oracle.sr_oracle_torch import TorchSR
    if srcfd.device_count() < 1:
        pytest.fail("gpu-marked test on a box without a HIP device")
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        rc, recs, err = _bench(["--steps", "3", "--warmup", "1", "--fields", "8", "--dump-outputs", str(d)])
        assert rc == 0, err[-2000:]
        r = recs[0]
        assert all(k in r for k in HEADLINE_KEYS), r
        assert not any(k in r for k in FULL_ONLY_KEYS), sorted(r)
        assert r["steps"] == 3 and r["dtype"] == "bf16" and r["higher_is_better"] is True and r["ms_per_step"] > 0 and r["nonfinite"] == 0
        assert r["value"] == pytest.approx(8 / (r["ms_per_step"] * 1e-3), rel=1e-3)
        y, idx = np.load(d / "y.npy"), np.load(d / "y_sample_index.npy")
        assert y.dtype == np.float32 and y.shape == (24, 400, 400, 1) and np.array_equal(idx, np.arange(24))
        dumps.append(y)
    assert np.array_equal(dumps[0], dumps[1])
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    synth = importlib.import_module("sr-for-cfd_amd.synth")
    lr, hr = srcfd.load_stats(STATS_TXT, 10, 400)
    x, ain, aout = bench.build_inputs(8, seed=0, stats_lr=lr, stats_hr=hr)
    enc_w = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1).weights()
    k = 6
    xs = (x[:k] - ain[:k, 0].reshape(-1, 1, 1, 1)) / ain[:k, 1].reshape(-1, 1, 1, 1)
    ref = TorchSR(enc_w, synth.synthetic_decoder_weights(1), torch.float64).forward(xs.astype(np.float32).astype(np.float64), batch_size=k)
    ys = (dumps[0][:k].astype(np.float64) - aout[:k, 0].reshape(-1, 1, 1, 1)) / aout[:k, 1].reshape(-1, 1, 1, 1)
    rel = np.linalg.norm((ys - ref).reshape(k, -1), axis=1) / np.linalg.norm(ref.reshape(k, -1), axis=1)
    assert rel.max() < 2e-2, rel
