"""The convergence summary of a benchmark-sized trace: the device call against the host estimators the benchmark uses.

    python tools/summary_bench.py [--out profiles/summary_bench.json] [--small] [--timeout 300]

Shapes: 4 chains x 1000 draws x 10 000 parameters and 8 x 1000 x 10 000 (the benchmark model's n), AR(1) draws with coefficient 0.5
from a fixed seed.  Per shape:

  * `pymc_amd.summary.summarize` -- all nine columns, the upload of the (chains, draws, P) host array included -- as
    device-synchronised wall time (the call returns host arrays) after one warm-up call on a 64-parameter slice, best of three;
  * `stats.ess_bulk_many` + `stats.rhat_many` on the host for the same array: TWO of the nine columns, the only ones the host has;
  * the largest difference between the two in those columns.

Every device measurement runs in a child process of its own under `--timeout` seconds, and the tool stops at the first one that
fails.  `--small` runs 4 x 1000 x 256 only (a smoke run of the tool itself).
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def trace(C, N, P, seed=0):
    from scipy.signal import lfilter

    e = np.random.default_rng(seed).standard_normal((C, N, P))
    return np.ascontiguousarray(lfilter([1.0], [1.0, -0.5], e, axis=1))


def child(C, N, P):
    from pymc_amd import stats, summary

    x = trace(C, N, P)
    summary.summarize(x[:, :, :64], device=0)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = summary.summarize(x, device=0)
        times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    e, r = stats.ess_bulk_many(x), stats.rhat_many(x)
    host = time.perf_counter() - t0
    out = {
        "chains": C, "draws": N, "parameters": P, "upload_bytes": int(x.nbytes),
        "device_all_columns_s": min(times), "device_all_columns_s_runs": times,
        "host_ess_bulk_and_rhat_s": host, "host_over_device": host / min(times),
        "ess_bulk_max_rel_diff": float(np.max(np.abs(got["ess_bulk"] / e - 1.0))), "r_hat_max_abs_diff": float(np.max(np.abs(got["r_hat"] - r))),
        "min_ess_bulk": float(got["ess_bulk"].min()), "max_r_hat": float(got["r_hat"].max()),
    }
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_bench.json"))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--timeout", type=int, default=300, help="seconds each device measurement may take")
    ap.add_argument("--child", nargs=3, type=int, metavar=("C", "N", "P"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(*a.child)
        return 0
    shapes = [(4, 1000, 256)] if a.small else [(4, 1000, 10_000), (8, 1000, 10_000)]
    res = {"small": bool(a.small), "shapes": []}
    for C, N, P in shapes:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(C), str(N), str(P)], capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"{C} x {N} x {P}: no result within {a.timeout} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"{C} x {N} x {P}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        res["shapes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(res["shapes"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
