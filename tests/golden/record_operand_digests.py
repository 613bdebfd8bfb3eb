"""Regenerates tests/golden/operand_pack_digests.json from the host harness (tools/pack_digest.cpp), for an INTENTIONAL change of an
operand layout.  The initial values were not produced this way: they were taken from commit 166b6e2, whose engine, 16-bit path and
trainer hashed every host buffer in front of its host-to-device copy (a scratch patch, not in the tree; that run had host stand-ins
for the device allocation and copy calls -- the buffers do not depend on the device), so the file pins the packers to what that
commit uploaded.  Regenerating it replaces that evidence by the harness's own output: say so in the commit
that does it, and let the GPU parity and error-map tests vouch for the new layout.

    python tests/golden/record_operand_digests.py
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


def main():
    pkg = importlib.import_module("sr-for-cfd_amd")
    synth = importlib.import_module("sr-for-cfd_amd.synth")
    enc = os.path.join(HERE, "vanilla_encoder10_to_400_swish_trained_upto_700_multiBC.h5")
    enc_w = pkg.SRModel.load_h5(enc, None, device=-1).weights()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sr-for-cfd_amd", "csrc"), "pack_digest"])
    with tempfile.TemporaryDirectory() as tmp:
        h5 = os.path.join(tmp, "superres.h5")
        pkg.SRModel.from_weights(enc_w, synth.synthetic_decoder_weights(1), device=-1).save_superres_h5(h5)
        out = subprocess.check_output([os.path.join(ROOT, "sr-for-cfd_amd", "lib", "pack_digest_asan"), h5], text=True)
    sections = {s["name"]: {"off": s["off"], "len": s["len"], "sha256": s["sha256"]} for s in json.loads(out)["sections"]}
    head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True).strip()
    doc = {"source": f"tools/pack_digest.cpp at {head} (regenerated; the initial values came from commit 166b6e2's upload sites)", "sections": sections}
    with open(os.path.join(HERE, "operand_pack_digests.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(sections)} sections")


if __name__ == "__main__":
    main()
