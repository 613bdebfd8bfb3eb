"""Sizes of the f32-grade forward's workspace on host-only handles (no GPU): srcfd_model_footprint and srcfd_model_workspace
against tests/golden/f32_workspace.json, recorded by tests/golden/record_f32_workspace.py on the commit that file names with the
handle's precision equal to the one asked about.  The sizes follow from the kernel choice (the streaming tail materialises nothing
behind ConvT#1; the bring-up path and SRCFD_NO_TAIL32=1 materialise every layer), so a reorganisation of that choice must not move
them; and an explicit precision argument decides alone, whatever the handle's own precision is."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from conftest import ENCODER_H5, GOLDEN

RECORDED_ON = "cbb7d7b"
NS = (0, 1, 3, 768, 2000)
PRECISIONS = ("fp32", "fp32x3", "fp32_naive")
DECODERS = (400, 80)
GOLDEN_JSON = os.path.join(GOLDEN, "f32_workspace.json")


def sweep(srcfd):
    """{"decoder_<hr>/handle=<h>/arg=<p>/n=<n>": [device_workspace, device_weights, staging, host_result, chunk, workspace bytes]}
    under the process's environment; the last two are srcfd_model_workspace's, which answers for the handle's precision."""
    L = importlib.import_module("sr-for-cfd_amd._lib")
    enc_w = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1).weights()
    rows = {}
    for hr in DECODERS:
        dec_w = (importlib.import_module("sr-for-cfd_amd.synth").synthetic_decoder_weights(1) if hr == 400
                 else importlib.import_module("sr-for-cfd_amd.family").synthetic_decoder_weights(hr))
        m = srcfd.SRModel.from_weights(enc_w, dec_w, device=-1)
        for h in PRECISIONS:
            m.precision = h
            for n in NS:
                nbytes = C.c_size_t(0)
                chunk = L.check(L.lib.srcfd_model_workspace(m._h, n, C.byref(nbytes)))
                for p in PRECISIONS:
                    fp = m.footprint(n, p)
                    rows[f"decoder_{hr}/handle={h}/arg={p}/n={n}"] = [fp["device_workspace"], fp["device_weights"], fp["device_host_entry_staging"],
                                                                      fp["host_result"], chunk, int(nbytes.value)]
        m.close()
    return rows


def sweep_in_child(env):
    """The sweep in a fresh process with `env` added: the recorded commit read SRCFD_NO_TAIL32 once per process."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **env), check=True, stdout=subprocess.PIPE, text=True).stdout
    return json.loads(next(l for l in out.splitlines() if l.startswith("{")))


def check(rows, golden):
    for key, row in rows.items():
        dec, h, p, n = key.split("/")
        want_fp = golden[f"{dec}/{p[len('arg='):]}/{n}"]      # footprint: the argument's precision decides ...
        want_ws = golden[f"{dec}/{h[len('handle='):]}/{n}"]   # ... srcfd_model_workspace has no such argument: the handle's
        assert row[:4] == want_fp[:4], (key, row, want_fp)
        assert row[4:] == want_ws[4:], (key, row, want_ws)


def _golden(which):
    doc = json.load(open(GOLDEN_JSON))
    assert doc["commit"] == RECORDED_ON
    return doc[which]


def test_f32_workspace_sizes_are_the_recorded_ones(srcfd):
    assert "SRCFD_NO_TAIL32" not in os.environ
    rows = sweep(srcfd)
    assert len(rows) == len(DECODERS) * len(PRECISIONS) ** 2 * len(NS)
    check(rows, _golden("default"))
    # decoder_400 at 768 samples: ConvT#1's output is the largest tensor the streaming tail leaves to materialise, one pass
    assert rows["decoder_400/handle=fp32/arg=fp32/n=768"][0] == 2 * 768 * 160000 * 4
    assert rows["decoder_400/handle=fp32/arg=fp32_naive/n=768"][0] > rows["decoder_400/handle=fp32/arg=fp32/n=768"][0]


def test_f32_workspace_sizes_without_the_streaming_tail():
    check(sweep_in_child({"SRCFD_NO_TAIL32": "1"}), _golden("SRCFD_NO_TAIL32=1"))


if __name__ == "__main__":
    import srcfd_amd
    print(json.dumps(sweep(srcfd_amd), sort_keys=True))
