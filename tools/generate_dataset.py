"""Writes the training-data file of sr-simulation-data-creation.ipynb cell 2 on the device: every Reynolds number on every mesh size,
batched across Reynolds numbers (datasets.generate_simulation_file).  Prints one line per run and a JSON summary.

    python tools/generate_dataset.py simulation_result_double_lid.h5 [--reynolds 100,200,...] [--mesh-sizes 10,50,400]
        [--bc double_lid|single_lid] [--dt 0.001] [--scheme QUICK] [--tolerance 1e-6] [--max-iterations 100000] [--max-batch 8]
        [--resident no|yes|auto]
"""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STATUS = {0: "reached max_iterations", 1: "converged", 2: "diverged, not written"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--reynolds", default=",".join(str(r) for r in range(100, 801, 100)))
    ap.add_argument("--mesh-sizes", default="10,50,400")
    ap.add_argument("--bc", choices=("double_lid", "single_lid"), default="double_lid")
    ap.add_argument("--dt", type=float, default=0.001)
    ap.add_argument("--scheme", choices=("QUICK", "UPWIND"), default="QUICK")
    ap.add_argument("--tolerance", type=float, default=1e-6)
    ap.add_argument("--max-iterations", type=int, default=100000)
    ap.add_argument("--max-batch", type=int, default=8)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--resident", choices=("no", "yes", "auto"), nargs="?", const="auto", default="no",
                    help="resident mode for the small meshes (at most 64 x 64): 'yes' refuses larger ones, 'auto' (also the bare flag) "
                         "runs them launch per sweep")
    a = ap.parse_args()
    datasets = importlib.import_module("sr-for-cfd_amd.datasets")
    coarse = importlib.import_module("sr-for-cfd_amd.coarse")
    bc, bc_type, case_name = {
        "double_lid": (coarse.LDC_DOUBLE_LID, "double_lid(u_top=1,u_bottom=1)", "double lid driven cavity"),
        "single_lid": (coarse.LDC_SINGLE_LID, "single_lid(u_top=1)", "lid driven cavity"),
    }[a.bc]
    t0 = time.time()
    record = datasets.generate_simulation_file(
        a.path, [int(r) for r in a.reynolds.split(",")], [int(n) for n in a.mesh_sizes.split(",")], bc=bc, bc_type=bc_type,
        case_name=case_name, dt=a.dt, scheme=a.scheme, convergence_criteria={c: a.tolerance for c in "uvp"},
        max_iterations=a.max_iterations, max_batch=a.max_batch, device=a.device,
        resident={"no": False, "yes": True, "auto": "auto"}[a.resident])
    for Re, n, iterations, status in record:
        print(f"Re {Re} mesh {n}x{n}: {iterations} iterations, {STATUS[status]}")
    print(json.dumps({"path": a.path, "runs": len(record), "written": sum(s != 2 for *_, s in record), "seconds": round(time.time() - t0, 1)}))
    return 0 if all(s != 2 for *_, s in record) else 1


if __name__ == "__main__":
    sys.exit(main())
