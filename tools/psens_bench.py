"""Power-scaling sensitivity at the benchmark's size: the device calls against the NumPy reference on the host, and a draw's
log-density total next to a WAIC draw.

    python tools/psens_bench.py [--out profiles/psens_bench.json] [--small] [--timeout 600]

Legs, each in a child process of its own under `--timeout` seconds (the tool stops at the first one that fails):

  * `psens 4` / `psens 8`: 4 x 1000 x 10 000 and 8 x 1000 x 10 000 draws (standard normal from a fixed seed; the component's
    log-density follows two of the parameters).  `sensitivity.psens_from_arrays` -- both weight calls and `nuts_psens`, the upload of
    the host array included -- as device-synchronised wall time after a warm-up call on a 64-parameter slice, best of three; the
    NumPy reference (tests/psens_reference.py) on the host over the first `--host-parameters` parameters (its time is per parameter:
    the figure for all 10 000 is that time scaled, and is marked as scaled); the largest |D - reference| over those parameters.
  * `logdens c2l` / `logdens glm`: C2-L (10 000 parameters, 4 992 000 rows) and the GLM shape (1 000 000 x 512, Bernoulli):
    `nuts_model_logdens_sum` of the observed node over 64 draws against a `nuts_waic_update` of the same 64 draws, per draw, each
    after a warm-up of 8 draws.

No time bar: the numbers are written down.  `--small` shrinks every shape by 16 (a smoke run of the tool itself).
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


def child_psens(C, N, P, host_p):
    import psens_reference as ps

    from pymc_amd import sensitivity

    rng = np.random.default_rng(0)
    x = rng.standard_normal((C, N, P))
    lc = -0.5 * (x[..., 0] - 1.0) ** 2 * 3.0 + 0.5 * x[..., 1] + 0.1 * rng.standard_normal((C, N))
    sensitivity.psens_from_arrays(x[:, :, :64], lc, device=0)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = sensitivity.psens_from_arrays(x, lc, device=0)
        times.append(time.perf_counter() - t0)
    host_p = min(host_p, P)
    t0 = time.perf_counter()
    ref = ps.psens_arrays(x.reshape(-1, P)[:, :host_p], lc.ravel())
    host = time.perf_counter() - t0
    out = {
        "leg": "psens", "chains": C, "draws": N, "parameters": P, "upload_bytes": int(x.nbytes),
        "device_s": min(times), "device_s_runs": times,
        "host_reference_parameters": host_p, "host_reference_s": host, "host_reference_s_scaled_to_all_parameters": host * P / host_p,
        "scaled_host_over_device": host * P / host_p / min(times),
        "max_abs_diff_in_D": float(max(np.max(np.abs(got[c][:host_p] ** 2 - ref[c] ** 2)) for c in ("cjs_lo", "cjs_hi"))),
        "khat": [got["khat_lo"], got["khat_hi"]], "khat_reference": [ref["khat_lo"], ref["khat_hi"]],
        "max_sensitivity": float(np.max(got["sensitivity"])), "median_sensitivity": float(np.median(got["sensitivity"])),
    }
    print(json.dumps(out), flush=True)


def child_logdens(shape, div):
    from pymc_amd import models
    from pymc_amd import model_spec as ms
    from pymc_amd.value_grad import DeviceValueGradFunction

    if shape == "c2l":
        spec = models.hier_logit(G=1248, D=8, rows_per_group=4000 // div)
    else:
        spec = models.glm_nuts(N=1_000_000 // div, P=512, family="bernoulli")
    name, kind, index, size = ms.observed_nodes(spec)[0]
    S = 64
    q = np.random.default_rng(1).normal(size=(S, spec.n)) * 0.1
    f = DeviceValueGradFunction(spec, device=0)
    try:
        f.logdens_sum(q[:8], (kind, index))
        t0 = time.perf_counter()
        tot = f.logdens_sum(q, (kind, index))
        t_sum = time.perf_counter() - t0
        acc = f.waic_accumulator(name, node=(kind, index))
        try:
            acc.update(q[:8])
            t0 = time.perf_counter()
            acc.update(q)
            acc.raw()
            t_waic = time.perf_counter() - t0
        finally:
            acc.close()
    finally:
        f.close()
    out = {"leg": "logdens", "shape": shape, "parameters": int(spec.n), "observed_rows": int(size), "draws": S,
           "logdens_sum_s_per_draw": t_sum / S, "waic_update_s_per_draw": t_waic / S, "logdens_sum_over_waic": t_sum / t_waic,
           "bytes_the_host_receives_per_draw": 8, "bytes_of_the_pointwise_row": 8 * int(size), "mean_total": float(np.mean(tot))}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psens_bench.json"))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--timeout", type=int, default=600, help="seconds each leg may take")
    ap.add_argument("--host-parameters", type=int, default=200, help="parameters the host reference is timed over")
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "psens":
            child_psens(*(int(v) for v in a.child[1:5]))
        else:
            child_logdens(a.child[1], int(a.child[2]))
        return 0
    div = 16 if a.small else 1
    legs = [["psens", "4", "1000", str(10_000 // div), str(a.host_parameters)], ["psens", "8", "1000", str(10_000 // div), str(a.host_parameters)],
            ["logdens", "c2l", str(div)], ["logdens", "glm", str(div)]]
    res = {"small": bool(a.small), "command": "python tools/psens_bench.py" + (" --small" if a.small else ""), "legs": []}
    for leg in legs:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + leg, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"{leg}: no result within {a.timeout} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"{leg}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        res["legs"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(res["legs"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
