"""Wall time of the prior draws next to the replicate pass they feed.

    python tools/prior_bench.py [--out profiles/prior_bench.json] [--small] [--timeout 900]

Shapes: C2-L (`models.hier_logit` with 4000 rows per group: 10 000 parameters, 4 992 000 observed rows) and
`models.hier_logit_variant("extra")` at the default G.  Per shape, in one process: `nuts_model_prior` for S = 64 after a warm-up
call, three calls, all three reported; then `nuts_model_predictive` of the observed rows over the same 64 positions, once after a
warm-up call of 8 rows.  Wall time, device-synchronised (both calls return host arrays).  No time bar: the numbers are written down.

Every shape runs in a child process of its own under `--timeout` seconds, and the tool stops at the first one that fails.
`--small` runs C2 at 40 rows per group and G = 32 only (a smoke run of the tool itself).
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

S = 64


def child(shape):
    from pymc_amd import models, predictive
    from pymc_amd.value_grad import DeviceValueGradFunction

    if shape == "c2l":
        spec = models.hier_logit(G=1248, D=8, rows_per_group=4000)
    elif shape == "extra":
        spec = models.hier_logit_variant("extra")
    else:
        spec = models.hier_logit_variant("extra", G=32, rows_per_group=40)
    plan = predictive.prior_plan(spec)
    f = DeviceValueGradFunction(spec, device=0)
    try:
        f.prior(S, seed=1)
        times = []
        for k in range(3):
            t0 = time.perf_counter()
            q, bad = f.prior(S, seed=2 + k)
            times.append(time.perf_counter() - t0)
        f.posterior_predictive("y", q[:8], seed=2)
        t0 = time.perf_counter()
        y = f.posterior_predictive("y", q, seed=2)
        t_pp = time.perf_counter() - t0
    finally:
        f.close()
    out = {"shape": shape, "parameters": int(spec.n), "levels": len(plan), "variables_per_level": [len(lv) for lv in plan], "draws": S,
           "observed_rows": int(y.shape[1]), "prior_s_runs": times, "prior_s_best": min(times), "predictive_s": t_pp,
           "predictive_over_prior": t_pp / min(times), "n_nonfinite": int(bad), "replicate_mean": float(np.mean(y))}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior_bench.json"))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--timeout", type=int, default=900, help="seconds each shape may take (C2-L's rows take a minute to draw)")
    ap.add_argument("--child", metavar="SHAPE", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    res = {"small": bool(a.small), "shapes": []}
    for shape in (["small"] if a.small else ["extra", "c2l"]):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape], capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"{shape}: no result within {a.timeout} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"{shape}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        res["shapes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(res["shapes"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
