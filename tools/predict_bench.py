"""Predictions at new data at the benchmark's shapes: what one streamed draw of `predictive.predict` costs, next to a WAIC draw and
a `ppc` draw.

    python tools/predict_bench.py [--draws 64] [--out profiles/predict_bench.json] [--small] [--parent parent.json]

At configs[3]'s GLM shape (1 M rows x 512 covariates, Bernoulli) and at C2-L (hierarchical-logit rows, 4 992 000 rows), with M = the
training rows (`model_spec.with_data` fed the training data: the kernels see the same rows the log-likelihood sees), on one GPU in
one process, device-synchronised wall time after a warm-up call:

  * `nuts_pred_update` with held-out values (moments and lpd folded) and without (moments only),
  * `nuts_waic_update` and `nuts_ppc_update` over the same draws in the same run,
  * `nuts_model_predict_moments` (the [S][N] conditional means travel to the host: the `expected` matrix).

`--parent FILE`: the output of `tools/loglik_bench.py --predictive` run at the parent commit on the same machine in the same
session; its WAIC and `ppc` figures are copied next to this run's and the ratios are also given against them.

By the shapes a streamed draw moves what WAIC's moves -- one read of X per batch of B and the 8 N-byte stage written and read --
with six accumulator rows instead of four: 16 N + 96 N / B bytes beside X against 16 N + 64 N / B (28 N against 24 N at B = 8).
`--small` runs both shapes at 1/16 size (a smoke run of the tool itself).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _wall(fn, reps=1):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def measure(spec, name, draws, seed=0):
    from pymc_amd.value_grad import DeviceValueGradFunction

    f = DeviceValueGradFunction(spec, device=0)
    q = np.random.default_rng(seed).normal(size=(draws, spec.n)) * 0.1
    out = {}
    try:
        B = int(f.model_scalar("loglik_batch"))

        def once(make):
            def run():
                acc = make()
                acc.update(q)
                acc.close()
            return run

        legs = {"waic": once(lambda: f.waic_accumulator(name)), "ppc": once(lambda: f.ppc_accumulator(name, seed=1)),
                "predict": once(lambda: f.pred_accumulator(name, with_y=True)), "predict_no_y": once(lambda: f.pred_accumulator(name, with_y=False))}
        for k, run in legs.items():
            run()                                              # warm-up: buffers, first launches
            out[k + "_us_per_draw"] = 1e6 * _wall(run, reps=3) / draws
        f.predict_moments(name, q[:B], var=False)
        out["moments_us_per_draw"] = 1e6 * _wall(lambda: f.predict_moments(name, q, var=False)) / draws
        out["batch"] = B
    finally:
        f.close()
    for k in ("predict", "predict_no_y", "moments"):
        out[k + "_over_waic"] = out[k + "_us_per_draw"] / out["waic_us_per_draw"]
        out[k + "_over_ppc"] = out[k + "_us_per_draw"] / out["ppc_us_per_draw"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_bench.json"))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent", default=None, help="output of `tools/loglik_bench.py --predictive` at the parent commit, same machine, same session")
    a = ap.parse_args()
    from pymc_amd import models
    from pymc_amd.model_spec import with_data

    parent = json.load(open(a.parent)) if a.parent else {}
    div = 16 if a.small else 1
    res = {"draws": a.draws, "small": bool(a.small)}
    N, P = 1_000_000 // div, 512
    G, D, rpg = 1248, 8, 4000 // div
    Nr = G * rpg

    def finish(key, r, n_rows, x_bytes):
        B = r["batch"]
        x_bytes = x_bytes(B)
        r.update(N=n_rows, bytes_per_draw_waic=x_bytes + 16 * n_rows + 64 * n_rows / B, bytes_per_draw_predict=x_bytes + 16 * n_rows + 96 * n_rows / B)
        r["predict_over_waic_by_the_bytes"] = r["bytes_per_draw_predict"] / r["bytes_per_draw_waic"]
        for k in ("waic", "ppc"):
            if parent.get(key, {}).get(k + "_us_per_draw"):
                r["parent_" + k + "_us_per_draw"] = parent[key][k + "_us_per_draw"]
                r["predict_over_parent_" + k] = r["predict_us_per_draw"] / parent[key][k + "_us_per_draw"]
        res[key] = r
        print(json.dumps({key: r}), flush=True)

    spec = models.glm_nuts(N=N, P=P, family="bernoulli")
    new = with_data(spec, {"y": {"X": spec.glm_rows.X, "y": spec.glm_rows.y}})
    del spec
    finish("glm", measure(new, "y", a.draws), N, lambda B: 8 * N * P / B)
    del new
    spec = models.hier_logit(G=G, D=D, rows_per_group=rpg)
    r = spec.logit_rows
    new = with_data(spec, {"y": {"X": r.X, "group_idx": r.group_idx, "y": r.y}})
    del spec, r
    finish("c2l", measure(new, "y", a.draws), Nr, lambda B: 8 * Nr * (D - 1) + Nr)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
