"""Records tests/golden/lowp16_output_digests.json on an MI355X: the sha256 of the f32 output bytes of every case of
tests/test_gpu_lowp16_bits.py (and of each input array), together with the commit whose library produced them.  Run it on the
commit whose bits are to be kept, BEFORE a change that must not move them; re-record only for an intended change of a 16-bit
kernel's arithmetic, and say so in the commit that does it.

    python tests/golden/record_lowp16_outputs.py --commit $(git rev-parse --short HEAD) [--out FILE]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "lowp16_output_digests.json"))
    args = ap.parse_args()
    import srcfd_amd as srcfd
    import test_gpu_lowp16_bits as t
    from conftest import ENCODER_H5
    if srcfd.device_count() < 1:
        raise SystemExit("needs a HIP device")
    enc_w = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1).weights()
    cases = {}
    for case in t.CASES:
        (y, again), plan = t.run_case(srcfd, enc_w, case, predicts=2)
        assert t.sha256(y) == t.sha256(again), t.case_id(case)
        want = case[3]
        assert {k: plan.get(k) for k in want} == want, (t.case_id(case), plan)
        cases[t.case_id(case)] = {"input_sha256": t.sha256(t.case_input(case)), "output_sha256": t.sha256(y), "plan": plan}
        print(t.case_id(case), cases[t.case_id(case)]["output_sha256"][:16], plan, flush=True)
    doc = {"source": "tests/golden/record_lowp16_outputs.py: f32 outputs of SRModel.predict on an MI355X", "commit": args.commit, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out}")


if __name__ == "__main__":
    main()
