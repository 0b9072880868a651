"""Pointwise log-likelihood at the benchmark's shapes: what a draw costs, against one pass of the sampler's own kernel.

    python tools/loglik_bench.py [--draws 64] [--loo-draws 1000] [--out profiles/loglik_bench.json] [--small]
    python tools/loglik_bench.py --predictive [--draws 64] [--out profiles/predictive_bench.json] [--small]
    python tools/loglik_bench.py --loo-pit [--loo-draws 1000] [--out profiles/loo_pit_bench.json] [--small]

At configs[3]'s GLM shape (1 M rows x 512 covariates, Bernoulli) and at C2-L (hierarchical-logit rows, 4 992 000 rows), on one GPU
in one process:

  * `nuts_model_loglik` for `--draws` draws in ONE call (device-synchronised wall time after a warm-up call; the [S][N] result
    travels to the host, which is part of the call),
  * `nuts_waic_update` for the same draws (the streaming accumulators: nothing but the draws crosses PCIe),
  * the GLM kernel's own single-column instantiation (engine option NUTS_LL_B = 1) through the same `nuts_waic_update`,
  * the PARENT's dominant pass at that shape: `DeviceValueGradFunction.time_kernels` (HIP events around the row-streaming kernel
    of one logp + gradient),
  * the LOO leg: `--loo-draws` draws around the initial point through `nuts_psis_update`, per draw over the whole trace and
    separately over its first and last fifth (draws 0-199 and 800-999 of 1 000: the columns fill, against the steady state in
    which most values are rejected at the threshold), `nuts_psis_read` once (k_psis_finish and the three result vectors to the
    host), and `nuts_waic_update` over the same draws in the same run to stand next to it.

`--predictive` runs the posterior-predictive leg INSTEAD (pymc_amd/predictive.py): microseconds per draw of `nuts_ppc_update` (the
streaming checks: nothing but the draws crosses PCIe) and of `nuts_model_predictive` (the [S][N] replicates travel to the host),
with `nuts_waic_update` over the same draws in the same run next to them, and their ratios to it.  By the shapes a draw of the
predictive path moves what WAIC's moves (one read of X per batch of B) plus 16 N bytes: the row pass stores eta, k_pp_draw reads
it and stores the variate in its place.

`--loo-pit` runs the LOO-PIT leg INSTEAD (`predictive.loo_pit`): over `--loo-draws` draws around the initial point, microseconds per
draw of the SECOND pass (`nuts_loo_pit_update`: per batch the log-likelihood, the weights, the replicates, the fold), with
`nuts_waic_update`, `nuts_psis_update` (the first pass) and `nuts_ppc_update` over the same draws in the same run next to it, the
one-off `nuts_loo_pit_create` (k_psis_fit over every observation) and the read.  By the shapes a second-pass draw should cost about
one WAIC draw plus one predictive draw plus 24 N bytes (the weight block written and read, the accumulators): the figure reported
as `loo_pit_over_waic_plus_ppc`.

Reported per shape: microseconds per draw, the ratio to the parent's pass, and the bytes a draw moves by the shapes
(GLM: 8 N P / B + 8 N; rows: 8 N per draw written, X read once per draw: 8 N D_stored + N).  The claim to check is "a batch of B
draws costs about one read of X".  `--small` runs both shapes at 1/16 size (a smoke run of the tool itself).
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


def measure_loo(f, name, n, draws, seed=1):
    """The LOO leg on an open function: microseconds per draw of nuts_psis_update by phase, the finish, WAIC on the same draws."""
    q = np.random.default_rng(seed).normal(size=(draws, n)) * 0.1
    fifth = draws // 5
    out = {"loo_draws": draws}

    def waic_once():
        acc = f.waic_accumulator(name)
        acc.update(q)
        acc.close()

    out["loo_waic_us_per_draw"] = 1e6 * _wall(waic_once) / draws
    acc = f.psis_accumulator(name, draws)
    try:
        t_fill = _wall(lambda: acc.update(q[:fifth]))
        t_mid = _wall(lambda: acc.update(q[fifth:draws - fifth]))
        t_steady = _wall(lambda: acc.update(q[draws - fifth:]))
        out["psis_us_per_draw"] = 1e6 * (t_fill + t_mid + t_steady) / draws
        out["psis_us_per_draw_fill"] = 1e6 * t_fill / fifth
        out["psis_us_per_draw_steady"] = 1e6 * t_steady / fifth
        t0 = time.perf_counter()
        elpd, khat, lppd, _ = acc.read()
        out["psis_read_ms"] = 1e3 * (time.perf_counter() - t0)
        out["psis_K1"] = int(np.ceil(min(draws / 5.0, 3.0 * np.sqrt(draws)))) + 1
        out["psis_state_bytes"] = 8 * (out["psis_K1"] + 4) * elpd.size
        out["psis_khat_max"] = float(np.max(khat))
        out["psis_elpd_loo"] = float(np.sum(elpd))
    finally:
        acc.close()
    out["psis_steady_over_waic"] = out["psis_us_per_draw_steady"] / out["loo_waic_us_per_draw"]
    out["psis_over_waic"] = out["psis_us_per_draw"] / out["loo_waic_us_per_draw"]
    return out


def measure_predictive(spec, name, draws, seed=0):
    from pymc_amd.value_grad import DeviceValueGradFunction

    f = DeviceValueGradFunction(spec, device=0)
    q = np.random.default_rng(seed).normal(size=(draws, spec.n)) * 0.1
    out = {}
    try:
        B = int(f.model_scalar("loglik_batch"))
        _, ms_dom = f.time_kernels(q[0], reps=20)
        out["parent_pass_us"] = 1e3 * ms_dom

        def waic_once():
            acc = f.waic_accumulator(name)
            acc.update(q)
            acc.close()

        def ppc_once():
            acc = f.ppc_accumulator(name, seed=1)
            acc.update(q)
            acc.close()

        waic_once()
        out["waic_us_per_draw"] = 1e6 * _wall(waic_once, reps=3) / draws
        ppc_once()
        out["ppc_us_per_draw"] = 1e6 * _wall(ppc_once, reps=3) / draws
        f.posterior_predictive(name, q[:B], seed=1)
        out["predictive_us_per_draw"] = 1e6 * _wall(lambda: f.posterior_predictive(name, q, seed=1)) / draws
        out["batch"] = B
    finally:
        f.close()
    out["ppc_over_waic"] = out["ppc_us_per_draw"] / out["waic_us_per_draw"]
    out["predictive_over_waic"] = out["predictive_us_per_draw"] / out["waic_us_per_draw"]
    return out


def measure_loo_pit(spec, name, draws, seed=1):
    from pymc_amd.value_grad import DeviceValueGradFunction

    f = DeviceValueGradFunction(spec, device=0)
    q = np.random.default_rng(seed).normal(size=(draws, spec.n)) * 0.1
    out = {"loo_draws": draws}
    try:
        out["batch"] = int(f.model_scalar("loglik_batch"))

        def waic_once():
            acc = f.waic_accumulator(name)
            acc.update(q)
            acc.close()

        def ppc_once():
            acc = f.ppc_accumulator(name, seed=1)
            acc.update(q)
            acc.close()

        waic_once()                                        # warm-up: buffers, first launches
        out["waic_us_per_draw"] = 1e6 * _wall(waic_once) / draws
        ppc_once()
        out["ppc_us_per_draw"] = 1e6 * _wall(ppc_once) / draws
        first = f.psis_accumulator(name, draws)
        try:
            out["psis_us_per_draw"] = 1e6 * _wall(lambda: first.update(q)) / draws
            t0 = time.perf_counter()
            second = f.loo_pit_accumulator(first, seed=1)
            out["loo_pit_create_ms"] = 1e3 * (time.perf_counter() - t0)
            try:
                out["loo_pit_us_per_draw"] = 1e6 * _wall(lambda: second.update(q)) / draws
                t0 = time.perf_counter()
                p_lt, p_eq, mean, var, sum_w, sum_w2, n = second.read()
                out["loo_pit_read_ms"] = 1e3 * (time.perf_counter() - t0)
            finally:
                second.close()
            ok = ~np.isnan(sum_w)
            out["observations_with_a_fit"] = int(ok.sum())
            out["sum_w_max_abs_error"] = float(np.max(np.abs(sum_w[ok] - 1.0))) if ok.any() else None
            out["ess_min"] = float(np.min(1.0 / sum_w2[ok])) if ok.any() else None
            out["loo_pit_state_bytes"] = 8 * (7 + 6 + out["batch"]) * int(sum_w.size)
        finally:
            first.close()
    finally:
        f.close()
    out["loo_pit_over_waic"] = out["loo_pit_us_per_draw"] / out["waic_us_per_draw"]
    out["loo_pit_over_waic_plus_ppc"] = out["loo_pit_us_per_draw"] / (out["waic_us_per_draw"] + out["ppc_us_per_draw"])
    out["loo_pit_over_psis"] = out["loo_pit_us_per_draw"] / out["psis_us_per_draw"]
    return out


def measure(spec, name, draws, seed=0, loo_draws=0):
    from pymc_amd import _lib
    from pymc_amd.value_grad import DeviceValueGradFunction

    f = DeviceValueGradFunction(spec, device=0)
    q = np.random.default_rng(seed).normal(size=(draws, spec.n)) * 0.1
    out = {}
    try:
        B = int(f.model_scalar("loglik_batch"))
        ms_total, ms_dom = f.time_kernels(q[0], reps=20)
        out["parent_pass_us"] = 1e3 * ms_dom
        out["parent_logp_grad_us"] = 1e3 * ms_total
        f.log_likelihood(name, q[:B])                     # warm-up: buffers, first launches
        t = _wall(lambda: f.log_likelihood(name, q))
        out["loglik_us_per_draw"] = 1e6 * t / draws

        def waic_once():
            acc = f.waic_accumulator(name)
            acc.update(q)
            acc.close()

        waic_once()
        out["waic_us_per_draw"] = 1e6 * _wall(waic_once, reps=3) / draws
        if spec.glm_rows is not None:
            _lib.set_engine_option("NUTS_LL_B", 1)
            try:
                waic_once()
                out["waic_us_per_draw_B1"] = 1e6 * _wall(waic_once, reps=1) / draws
            finally:
                _lib.unset_engine_option("NUTS_LL_B")
        out["batch"] = B
        out["stage_bytes"] = int(f.model_scalar("loglik_stage_bytes"))
        if loo_draws:
            out.update(measure_loo(f, name, spec.n, loo_draws))
    finally:
        f.close()
    for k in ("loglik_us_per_draw", "waic_us_per_draw", "waic_us_per_draw_B1"):
        if k in out:
            out[k.replace("_us_per_draw", "_over_parent_pass")] = out[k] / out["parent_pass_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=64)
    ap.add_argument("--loo-draws", type=int, default=1000, help="draws of the LOO leg (0: skip it)")
    ap.add_argument("--out", default=None, help="default: profiles/loglik_bench.json (profiles/predictive_bench.json with --predictive)")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--predictive", action="store_true", help="the posterior-predictive leg instead of the log-likelihood legs")
    ap.add_argument("--loo-pit", action="store_true", help="the LOO-PIT leg (the second pass) instead of the log-likelihood legs")
    a = ap.parse_args()
    from pymc_amd import models

    a.out = a.out or os.path.join(ROOT, "profiles", "loo_pit_bench.json" if a.loo_pit else "predictive_bench.json" if a.predictive else "loglik_bench.json")
    div = 16 if a.small else 1
    res = {"draws": a.draws, "loo_draws": a.loo_draws, "small": bool(a.small)}
    N, P = 1_000_000 // div, 512
    G, D, rpg = 1248, 8, 4000 // div
    if a.loo_pit:
        res = {"loo_draws": a.loo_draws, "small": bool(a.small)}
        r = measure_loo_pit(models.glm_nuts(N=N, P=P, family="bernoulli"), "y", a.loo_draws)
        r.update(N=N, P=P, bytes_per_draw_waic=8 * N * P / r["batch"] + 8 * N, bytes_per_draw_ppc=8 * N * P / r["batch"] + 8 * N + 16 * N)
        r["bytes_per_draw_loo_pit"] = r["bytes_per_draw_waic"] + r["bytes_per_draw_ppc"] + 24 * N
        res["glm"] = r
        print(json.dumps({"glm": r}), flush=True)
        Nr = G * rpg
        r = measure_loo_pit(models.hier_logit(G=G, D=D, rows_per_group=rpg), "y", a.loo_draws)
        r.update(N=Nr, D=D, bytes_per_draw_waic=8 * Nr * (D - 1) + Nr + 8 * Nr, bytes_per_draw_ppc=8 * Nr * (D - 1) + Nr + 8 * Nr + 16 * Nr)
        r["bytes_per_draw_loo_pit"] = r["bytes_per_draw_waic"] + r["bytes_per_draw_ppc"] + 24 * Nr
        res["c2l"] = r
        print(json.dumps({"c2l": r}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
        return
    if a.predictive:
        res = {"draws": a.draws, "small": bool(a.small)}
        r = measure_predictive(models.glm_nuts(N=N, P=P, family="bernoulli"), "y", a.draws)
        r.update(N=N, P=P, bytes_per_draw_waic=8 * N * P / r["batch"] + 8 * N, bytes_per_draw_predictive=8 * N * P / r["batch"] + 8 * N + 16 * N)
        res["glm"] = r
        print(json.dumps({"glm": r}), flush=True)
        Nr = G * rpg
        r = measure_predictive(models.hier_logit(G=G, D=D, rows_per_group=rpg), "y", a.draws)
        r.update(N=Nr, D=D, bytes_per_draw_waic=8 * Nr * (D - 1) + Nr + 8 * Nr, bytes_per_draw_predictive=8 * Nr * (D - 1) + Nr + 8 * Nr + 16 * Nr)
        res["c2l"] = r
        print(json.dumps({"c2l": r}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
        return
    spec = models.glm_nuts(N=N, P=P, family="bernoulli")
    r = measure(spec, "y", a.draws, loo_draws=a.loo_draws)
    r.update(N=N, P=P, bytes_per_draw=8 * N * P / r["batch"] + 8 * N, bytes_parent_pass=8 * N * P)
    res["glm"] = r
    print(json.dumps({"glm": r}), flush=True)
    del spec
    spec = models.hier_logit(G=G, D=D, rows_per_group=rpg)
    r = measure(spec, "y", a.draws, loo_draws=a.loo_draws)
    Nr = G * rpg
    r.update(N=Nr, D=D, bytes_per_draw=8 * Nr * (D - 1) + Nr + 8 * Nr, bytes_parent_pass=Nr * (8 * (D - 1) + 1))
    res["c2l"] = r
    print(json.dumps({"c2l": r}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
