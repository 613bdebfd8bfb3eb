"""Records tests/golden/family_pack_digests.json: the `family.*` sections of the host harness (tools/pack_digest.cpp) for the trained
multiBC encoder + family.synthetic_decoder_weights(hr), hr = 10 (the smallest graph) and hr = 80 (the one whose narrow-channel GEMM
runs) -- the weights of tests/test_model_family.py::test_pack_harness_family_mode_runs_clean, which compares against this file.
These are the host buffers of the f32 plan, of the 16-bit path of the family graphs (family.any16.*) and of the trainer's maps.
Run it on the commit whose bytes are to be kept, before a change that must not move them.

    python tests/golden/record_family_pack_digests.py
"""
import importlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
HRS = (10, 80)


def main():
    pkg = importlib.import_module("sr-for-cfd_amd")
    synth = importlib.import_module("sr-for-cfd_amd.synth")
    fam = importlib.import_module("sr-for-cfd_amd.family")
    enc = os.path.join(HERE, "vanilla_encoder10_to_400_swish_trained_upto_700_multiBC.h5")
    enc_w = pkg.SRModel.load_h5(enc, None, device=-1).weights()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sr-for-cfd_amd", "csrc"), "pack_digest"])
    files = {}
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "superres.h5")
        pkg.SRModel.from_weights(enc_w, synth.synthetic_decoder_weights(1), device=-1).save_superres_h5(base)
        for hr in HRS:
            h5, dump = os.path.join(tmp, f"superres_10to{hr}.h5"), os.path.join(tmp, f"dump{hr}")
            os.mkdir(dump)
            pkg.SRModel.from_weights(enc_w, fam.synthetic_decoder_weights(hr), device=-1).save_superres_h5(h5)
            out = subprocess.check_output([os.path.join(ROOT, "sr-for-cfd_amd", "lib", "pack_digest_asan"), base, dump, h5], text=True)
            files[f"decoder_{hr}"] = {s["name"]: {"off": s["off"], "len": s["len"], "sha256": s["sha256"]} for s in json.loads(out)["sections"]
                                      if s["name"].startswith("family.")}
            print(f"decoder_{hr}: {len(files[f'decoder_{hr}'])} sections")
    head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True).strip()
    doc = {"source": f"tools/pack_digest.cpp at {head}", "files": files}
    with open(os.path.join(HERE, "family_pack_digests.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
