"""Model comparison at the benchmark's sizes: the device calls against the bytes they must move and the NumPy restatement on the host.

    python tools/compare_bench.py [--out profiles/compare_bench.json] [--small] [--timeout 600]

Shapes: K = 4 random finite elpd vectors (`close` of tests/compare_reference.py) at N = 1 000 000 and N = 4 992 000 (C2-L).  Per shape,
device-synchronised wall times (every call returns host numbers), best of three unless said otherwise:

  * upload        the K `set` calls (host check for non-finite values, copy, scatter);
  * moments       `nuts_compare_moments` (two passes over e, four launches);
  * stacking      the whole solve, and ONE PASS as (wall time of repeated solves) / (passes they took), at least 100 passes after a
                  first solve as warm-up (which also computes the terms p) -- a pass is one k_cmp_stack_pass launch, one reduce launch
                  and a copy of K (K + 3) / 2 + 1 numbers, so this is the time per pass AS THE SOLVER SEES IT, host step included;
                  against 8 K N bytes, the p a pass must read;
  * bb            `nuts_compare_bb` at b_samples = 1000.

Host: the restatement's moments, one `stack_pass`, its whole `solve`, and `bb` at b_samples = 8 SCALED by 1000 / 8 (the figure is
marked as scaled: the host was not run at 1000).  `--small` runs N = 100 000 only (a smoke run of the tool itself).

Every shape runs in a child process of its own under `--timeout` seconds, and the tool stops at the first one that fails.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

K = 4
B = 1000
B_HOST = 8


def best(fn, n=3):
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times), out


def child(N):
    import compare_reference as cr
    from pymc_amd import compare as cmp

    e = cr.make(N, K, 1, "close")
    cols = [np.ascontiguousarray(e[:, k]) for k in range(K)]
    out = {"N": N, "K": K, "b_samples": B, "state_bytes": 16 * K * N, "pass_bytes": 8 * K * N}
    with cmp.Comparison(N, K, device=0) as c:
        out["upload_s"], _ = best(lambda: [c.set(k, cols[k]) for k in range(K)])
        out["moments_s"], mom = best(c.moments)
        w, f, gap, passes = c.stacking()                      # warm-up; fills p
        out["stacking_solve_s"], (w, f, gap, passes) = best(c.stacking)
        out["stacking_passes"], out["stacking_kkt_gap"] = passes, gap
        done, t0 = 0, time.perf_counter()
        while done < 100:
            done += c.stacking()[3]
        dt = time.perf_counter() - t0
        out["stacking_pass_s"], out["stacking_pass_measured_over"] = dt / done, done
        out["stacking_pass_GBps"] = 8 * K * N / (dt / done) / 1e9
        c.bb(8, 0)
        out["bb_s"], (wb, seb) = best(lambda: c.bb(B, 0), n=2)
    t0 = time.perf_counter()
    mom0 = cr.moments(e)
    out["host_moments_s"] = time.perf_counter() - t0
    m, p = cr.terms(e)
    out["host_stack_pass_s"], _ = best(lambda: cr.stack_pass(p, np.full(K, 1.0 / K)))
    t0 = time.perf_counter()
    w0, f0, gap0, passes0 = cr.solve(e, tol=1e-10)
    out["host_stacking_solve_s"], out["host_stacking_passes"] = time.perf_counter() - t0, passes0
    t0 = time.perf_counter()
    cr.bb(e, B_HOST, 0, block=B_HOST)
    host8 = time.perf_counter() - t0
    out["host_bb_s_at_8_replicates"] = host8
    out["host_bb_s_scaled_to_1000"] = host8 * B / B_HOST          # SCALED, not measured
    out["moments_max_rel_diff"] = float(max(np.max(np.abs(mom[j] / mom0[j] - 1.0)) for j in range(2)))
    out["stacking_weight_max_abs_diff"] = float(np.abs(w - w0).max())
    out["stacking_objective_rel_diff"] = abs(f - f0) / abs(f0)
    out["host_over_device_moments"] = out["host_moments_s"] / out["moments_s"]
    out["host_over_device_stack_pass"] = out["host_stack_pass_s"] / out["stacking_pass_s"]
    out["host_over_device_stacking_solve"] = out["host_stacking_solve_s"] / out["stacking_solve_s"]
    out["host_over_device_bb_scaled"] = out["host_bb_s_scaled_to_1000"] / out["bb_s"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_bench.json"))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--timeout", type=int, default=600, help="seconds each shape may take")
    ap.add_argument("--child", type=int, metavar="N", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    res = {"small": bool(a.small), "shapes": []}
    for N in ([100_000] if a.small else [1_000_000, 4_992_000]):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(N)], capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"N = {N}: no result within {a.timeout} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"N = {N}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        res["shapes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(res["shapes"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
