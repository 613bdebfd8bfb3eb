"""Records tests/golden/train_step_digests.json on an MI355X: for every case of tests/test_gpu_train_step_bits.py the sha256 of
the inputs (x, y, initial parameters), the sha256 of the flat gradient and the bits of the squared-error sum, together with the
commit whose library produced them.  Run it on the commit whose gradient bits are to be kept, BEFORE a change that must not move
them; re-record only for an intended change of a training kernel's arithmetic, and say so in the commit that does it.  Every case
runs in a fresh child process, one after the other; the four calls of a case (plain, capture, replay, overwrite) must already
agree on the recorded commit.

    python tests/golden/record_train_step.py --commit $(git rev-parse --short HEAD) [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def record_case(cid):
    import srcfd_amd as srcfd
    import test_gpu_train_step_bits as t
    from conftest import ENCODER_H5
    from oracle import sr_oracle
    if srcfd.device_count() < 1:
        raise SystemExit("needs a HIP device")
    case = next(c for c in t.CASES if t.case_id(c) == cid)
    enc_w = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1).weights()
    inputs, got = t.run_case(srcfd, enc_w, sr_oracle.synthetic_decoder(1), case)
    assert len(set(got)) == 1, (cid, got)
    return {"input_sha256": inputs, "grads_sha256": got[0][0], "sse_bits": got[0][1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "train_step_digests.json"))
    ap.add_argument("--case", help="(child process) record this case and print it as one JSON line")
    args = ap.parse_args()
    if args.case:
        print("CASE " + json.dumps(record_case(args.case), sort_keys=True), flush=True)
        return
    if not args.commit:
        ap.error("--commit is required")
    import test_gpu_train_step_bits as t
    cases = {}
    for case in t.CASES:
        cid = t.case_id(case)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", cid], stdout=subprocess.PIPE, text=True, timeout=120)
        if res.returncode != 0:   # a fault in one case: nothing more is started on the device
            raise SystemExit(f"{cid}: child exited with {res.returncode}\n{res.stdout}")
        line = next(l for l in res.stdout.splitlines() if l.startswith("CASE "))
        cases[cid] = json.loads(line[5:])
        print(cid, cases[cid]["grads_sha256"][:16], cases[cid]["sse_bits"], flush=True)
    doc = {"source": "tests/golden/record_train_step.py: gradients and squared-error sums of Trainer.forward_backward on an MI355X",
           "commit": args.commit, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out}")


if __name__ == "__main__":
    main()
