"""Records tests/golden/f32_forward_digests.json on an MI355X: for every case of tests/test_gpu_f32_forward_bits.py the sha256 of
the input, the sha256 of the f32 output bytes, the names of the launches (set_profiling / get_profile) and last_plan(), together
with the commit whose library produced them.  Run it on the commit whose bits and kernel choice are to be kept, BEFORE a change
that must not move them; re-record only for an intended change of an f32 kernel's arithmetic or of the choice, and say so in the
commit that does it.  Every case runs in a fresh child process, one after the other: the recorded commit read four of its
switches once per process.

    python tests/golden/record_f32_forward.py --commit $(git rev-parse --short HEAD) [--out FILE]
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
    import test_gpu_f32_forward_bits as t
    from conftest import ENCODER_H5
    if srcfd.device_count() < 1:
        raise SystemExit("needs a HIP device")
    case = next(c for c in t.CASES if t.case_id(c) == cid)
    enc_w = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1).weights()
    shas, plans, names = t.run_case(srcfd, enc_w, case)
    assert len(set(shas)) == 1, (cid, shas)
    assert [p["graph"] for p in plans] == (["eager", "capture", "replay"] if case[2] <= 96 else ["eager"] * 3), (cid, plans)
    return {"input_sha256": t.sha256(t.case_input(case)), "output_sha256": shas[0], "launches": names, "plan": dict(plans[0], graph="eager")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "f32_forward_digests.json"))
    ap.add_argument("--case", help="(child process) record this case and print it as one JSON line")
    args = ap.parse_args()
    if args.case:
        print("CASE " + json.dumps(record_case(args.case), sort_keys=True), flush=True)
        return
    if not args.commit:
        ap.error("--commit is required")
    import test_gpu_f32_forward_bits as t
    cases = {}
    for case in t.CASES:
        cid = t.case_id(case)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", cid], stdout=subprocess.PIPE, text=True, timeout=120)
        if res.returncode != 0:   # a fault in one case: nothing more is started on the device
            raise SystemExit(f"{cid}: child exited with {res.returncode}\n{res.stdout}")
        line = next(l for l in res.stdout.splitlines() if l.startswith("CASE "))
        cases[cid] = json.loads(line[5:])
        print(cid, cases[cid]["output_sha256"][:16], cases[cid]["launches"], flush=True)
    doc = {"source": "tests/golden/record_f32_forward.py: f32 outputs and launch names of SRModel.predict on an MI355X", "commit": args.commit, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out}")


if __name__ == "__main__":
    main()
