"""Records tests/golden/f32_workspace.json (no GPU needed): srcfd_model_footprint and srcfd_model_workspace of host-only handles
over the sweep of tests/test_f32_plan.py, with the handle's precision equal to the precision asked about, in the default
environment and under SRCFD_NO_TAIL32=1 (each in a fresh process).  Run it on the commit whose sizes are to be kept.

    python tests/golden/record_f32_workspace.py --commit $(git rev-parse --short HEAD) [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(HERE, "f32_workspace.json"))
    args = ap.parse_args()
    import test_f32_plan as t
    doc = {"source": "tests/golden/record_f32_workspace.py: [footprint's four sizes, srcfd_model_workspace's chunk and bytes] per decoder / precision / n",
           "commit": args.commit}
    for which, env in (("default", {}), ("SRCFD_NO_TAIL32=1", {"SRCFD_NO_TAIL32": "1"})):
        rows = t.sweep_in_child(env)
        doc[which] = {}
        for key, row in rows.items():
            dec, h, p, n = key.split("/")
            if h[len("handle="):] == p[len("arg="):]:   # the other rows are what the test derives
                doc[which][f"{dec}/{p[len('arg='):]}/{n}"] = row
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(doc['default'])} + {len(doc['SRCFD_NO_TAIL32=1'])} rows -> {args.out}")


if __name__ == "__main__":
    main()
