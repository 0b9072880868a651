"""Posterior predictive of a trace on the device: replicates y_rep per draw, and the streaming predictive checks.

`pm.sample_posterior_predictive(idata)` draws one replicate of every observed variable per posterior draw; `az.plot_ppc` /
`az.plot_bpv` then look at per-observation predictive means and p-values and at the distribution of test statistics T(y_rep) against
T(y).  Here the replicates come from the engine (csrc/predictive.h, csrc/predictive_kernel.h): `sample_posterior_predictive`
returns the arrays, `ppc` accumulates the per-observation and per-draw summaries on the device while the draws stream by and never
holds the (draws x observations) matrix -- the models this engine exists for have 10^6 observations.  `loo_pit` (`az.loo_pit`, the LOO
predictive mean and sd) weights the replicates by the Pareto-smoothed leave-one-out weights in a second streamed pass
(csrc/psis.h psis_fit / psis_weight, csrc/loo_pit_kernel.h).

The generator is counter-based: the value of (draw s, observation i) of a variable depends on (seed, variable, s, i) and on the
variable's parameters at draw s, never on how the draws were batched or split over calls.  s is the GLOBAL draw index: draw d of the model's
chain number c is c * draws + d, whichever process holds that chain.  The draws are what `sample()` returns: raveled, UNCONSTRAINED positions.
"""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from pymc_amd import loglik
from pymc_amd import model_spec as ms

REFUSED_FAMILIES = (ms.D_TRUNCNORMAL, ms.D_BINOMIAL, ms.D_POTENTIAL, ms.D_DERIVED)
STATS = ("mean", "sd", "min", "max")


def seed_from(random_seed) -> int:
    """The 64-bit key of the generator for `sample(random_seed=...)`."""
    return int(np.random.SeedSequence(random_seed).generate_state(1, np.uint64)[0])


def refusal(spec, nodes=None) -> Optional[str]:
    """Why replicates of `spec`'s observed `nodes` cannot be drawn from the continuous draws alone: `loglik.refusal`'s reasons, and
    the families no variate generator exists for."""
    why = loglik.refusal(spec, nodes)
    if why:
        return why
    for name, kind, index, _ in (ms.observed_nodes(spec) if nodes is None else nodes):
        if kind != ms.LL_FACTOR:
            continue
        f = spec.factors[index]
        if f.dist in REFUSED_FAMILIES:
            return f"{name!r} is a {ms.DIST_NAMES[f.dist]} factor: forward sampling of that family is out of scope"
        if any(op.kind not in (ms.OP_CONST, ms.OP_DATA) for op in (f.args[0].a, f.args[0].b, f.args[0].c)):
            return f"{name!r}: the factor's value is an expression of variables, not observed data"
    return None


def _chain_ids(draws, chain_ids, n_chains):
    if chain_ids is None and isinstance(draws, dict) and draws.get("chains") is not None:
        chain_ids = draws["chains"]
    ids = list(range(n_chains)) if chain_ids is None else [int(c) for c in chain_ids]
    if len(ids) != n_chains:
        raise ValueError(f"chain_ids names {len(ids)} chains, draws holds {n_chains}")
    return ids


def _nodes_or_refuse(spec, var_names):
    nodes = loglik._select(spec, var_names)
    why = refusal(spec, nodes)
    if why:
        raise ValueError("posterior predictive refused: " + why)
    return nodes


def sample_posterior_predictive(model, draws, *, var_names=None, random_seed=0, chain_ids=None, device: Optional[int] = None,
                                func=None) -> Dict[str, np.ndarray]:
    """`pm.sample_posterior_predictive`: {observed variable: (chains, draws, size)}, one replicate per draw, in the order the
    observations were passed.  `random_seed`: the generator's 64-bit key.  `chain_ids`: the model's chain number of each chain of
    `draws` (default 0, 1, ...; a result dict's own "chains" is used): chain number c's draw d is draw c * draws + d of the stream,
    so a rank that holds only some of the chains draws what a process holding all of them would.  `func`: a
    `DeviceValueGradFunction` of the spec to evaluate on (default: one is built on `device` and closed).  A model without observed
    variables gives {}."""
    spec = loglik._spec_of(model)
    nodes = _nodes_or_refuse(spec, var_names)
    if not nodes:
        return {}
    q = loglik._draws_array(draws, spec.n)
    ids = _chain_ids(draws, chain_ids, q.shape[0])
    f, own = loglik._function(spec, device, func)
    try:
        out = {}
        for name, kind, index, size in nodes:
            y = np.stack([f.posterior_predictive(name, q[k], seed=random_seed, draw0=c * q.shape[1], node=(kind, index)) for k, c in enumerate(ids)])
            out[name] = loglik.caller_order(spec, kind, y)
        return out
    finally:
        if own:
            f.close()


def ppc_from_accumulators(mean_i, var_i, n_lt_i, n_eq_i, T, T_obs, n_draws: int, pointwise: bool = False) -> dict:
    """The predictive checks from the streamed state of S = `n_draws` pooled draws over N observations: per draw the statistics
    T(y_rep) = mean, sd (population), min, max from T = [S, 4] (sum, sum of squares, min, max), the same four of the observed data
    from `T_obs`, and the Bayesian p-values P(T(y_rep) >= T(y)); with `pointwise` per observation mean_i, var_i and
    p_i = (#{y_rep < y_i} + 0.5 #{y_rep == y_i}) / S.

    NaN replicates are not hidden: a draw with a NaN replicate has NaN for all four statistics and makes the four p-values NaN; an
    observation with a NaN replicate at any draw has NaN mean_i, var_i and p_i."""
    T, T_obs = np.asarray(T, dtype="float64").reshape(-1, 4), np.asarray(T_obs, dtype="float64")
    N = int(np.size(mean_i))
    S = float(n_draws)

    def four(t):
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = t[..., 0] / N
            return {"mean": mean, "sd": np.sqrt(np.maximum(t[..., 1] / N - mean * mean, 0.0)), "min": t[..., 2], "max": t[..., 3]}

    rep, obs = four(T), four(T_obs)
    out = {"n_samples": int(n_draws), "n_data_points": N, "T_obs": {k: float(obs[k]) for k in STATS}}
    for k in STATS:
        out["T_" + k] = rep[k]
        out["p_" + k] = float(np.mean(rep[k] >= obs[k])) if len(T) and not np.any(np.isnan(rep[k])) else float("nan")
    if pointwise:
        out["mean_i"] = np.asarray(mean_i, dtype="float64")
        out["var_i"] = np.asarray(var_i, dtype="float64")
        p_i = (np.asarray(n_lt_i, dtype="float64") + 0.5 * np.asarray(n_eq_i, dtype="float64")) / S
        out["p_i"] = np.where(np.isnan(out["mean_i"]), np.nan, p_i)
    return out


def ppc(model, draws, *, var_name: Optional[str] = None, random_seed=0, pointwise: bool = False, device: Optional[int] = None, func=None) -> dict:
    """Streaming posterior-predictive checks of one observed variable with the chains pooled in chain order (see
    `ppc_from_accumulators`); the replicates are those `sample_posterior_predictive` returns under the same `random_seed`."""
    spec = loglik._spec_of(model)
    nodes = ms.observed_nodes(spec)
    why = loglik.refusal(spec, [])
    if why:
        raise ValueError("posterior predictive refused: " + why)
    if not nodes:
        raise ValueError("the model has no observed variable")
    if var_name is None and len(nodes) > 1:
        raise TypeError(f"Found several observed variables {[nd[0] for nd in nodes]}, var_name cannot be None")
    node = _nodes_or_refuse(spec, var_name)[0]
    q = loglik._draws_array(draws, spec.n)
    f, own = loglik._function(spec, device, func)
    try:
        acc = f.ppc_accumulator(node[0], seed=random_seed, node=(node[1], node[2]))
        try:
            for c in range(q.shape[0]):
                acc.update(q[c])
            mean_i, var_i, n_lt, n_eq, n_draws = acc.read()
            T, T_obs = acc.stats()
        finally:
            acc.close()
    finally:
        if own:
            f.close()
    mean_i, var_i, n_lt, n_eq = (loglik.caller_order(spec, node[1], a) for a in (mean_i, var_i, n_lt, n_eq))
    return ppc_from_accumulators(mean_i, var_i, n_lt, n_eq, T, T_obs, n_draws, pointwise=pointwise)


def loo_pit_from_accumulators(p_lt, p_eq, mean, var, sum_w, sum_w2, elpd_loo_i, khat_i, lppd_i, n_draws: int, pointwise: bool = True) -> dict:
    """The LOO predictive checks of N observations from the two streamed passes over S = `n_draws` pooled draws: the first pass's
    PSIS results (`loglik.loo_from_pointwise`, whose keys are all returned) and the second pass's weighted sums.

    loo_pit = p_lt + p_eq is ArviZ's `loo_pit` (the weight of y_rep <= y); loo_pit_mid = p_lt + p_eq / 2 is the mid-p value for
    discrete data, the LOO counterpart of `ppc`'s p_i; loo_mean and loo_sd are the LOO predictive mean and standard deviation
    (population, weighted); ess = 1 / sum w^2 the effective sample size of the weights; sum_w is 1 after a complete second pass.
    An observation whose fit is degenerate (ll = -inf at a draw) or poisoned (a NaN or +inf value) has NaN in all of them.

    Raises ValueError when an observation with a finite elpd_loo_i has |sum_w - 1| > 1e-9: the second pass streamed other draws
    than the first, or not all of them."""
    p_lt, p_eq, mean, var, sum_w, sum_w2 = (np.asarray(a, dtype="float64") for a in (p_lt, p_eq, mean, var, sum_w, sum_w2))
    ok = np.isfinite(np.asarray(elpd_loo_i, dtype="float64"))
    if np.any(~(np.abs(sum_w[ok] - 1.0) <= 1e-9)):
        raise ValueError("the second pass did not see the draws of the first")
    out = loglik.loo_from_pointwise(elpd_loo_i, khat_i, lppd_i, n_draws, pointwise=pointwise)
    with np.errstate(invalid="ignore", divide="ignore"):
        out.update({
            "loo_pit": p_lt + p_eq,
            "loo_pit_mid": p_lt + 0.5 * p_eq,
            "p_lt": p_lt,
            "p_eq": p_eq,
            "loo_mean": mean,
            "loo_sd": np.sqrt(var),
            "ess": 1.0 / sum_w2,
            "sum_w": sum_w,
        })
    return out


def loo_pit(model, draws, *, var_name: Optional[str] = None, reff: float = 1.0, random_seed=0, chain_ids=None, pointwise: bool = True,
            device: Optional[int] = None, func=None) -> dict:
    """`az.loo_pit` and the LOO predictive mean and sd of one observed variable, streamed: a first pass over the draws builds the
    PSIS state (`loglik.loo`), a second weights each draw's replicate by its Pareto-smoothed leave-one-out weight and folds per
    observation (see `loo_pit_from_accumulators`).  Neither the log-likelihood, the replicate nor the weight matrix
    (draws x observations) is ever formed.  The chains are pooled in chain order; the replicates are those
    `sample_posterior_predictive` returns under the same `random_seed` and `chain_ids`.  Arrays are in the order the observations
    were passed.  `pointwise=False` drops `loo_i` and `pareto_k` (as `loglik.loo` does), not the LOO-PIT arrays.

    Tied log-likelihood values of an observation share the mean of the weights of the ranks they occupy: the result does not depend
    on the order of the draws (ArviZ's does; the two agree when no value repeats)."""
    spec = loglik._spec_of(model)
    nodes = ms.observed_nodes(spec)
    why = loglik.refusal(spec, [])
    if why:
        raise ValueError("posterior predictive refused: " + why)
    if not nodes:
        raise ValueError("the model has no observed variable")
    if var_name is None and len(nodes) > 1:
        raise TypeError(f"Found several observed variables {[nd[0] for nd in nodes]}, var_name cannot be None")
    node = _nodes_or_refuse(spec, var_name)[0]
    q = loglik._draws_array(draws, spec.n)
    ids = _chain_ids(draws, chain_ids, q.shape[0])
    n_draws = q.shape[0] * q.shape[1]
    f, own = loglik._function(spec, device, func)
    try:
        first = f.psis_accumulator(node[0], n_draws, reff=reff, node=(node[1], node[2]))
        try:
            for c in range(q.shape[0]):
                first.update(q[c])
            elpd_i, khat, lppd_i, _ = first.read()
            second = f.loo_pit_accumulator(first, seed=random_seed)
            try:
                for k, c in enumerate(ids):
                    second.update(q[k], draw0=c * q.shape[1])
                cols = second.read()[:6]
            finally:
                second.close()
        finally:
            first.close()
    finally:
        if own:
            f.close()
    cols = [loglik.caller_order(spec, node[1], a) for a in cols]
    elpd_i, khat, lppd_i = (loglik.caller_order(spec, node[1], a) for a in (elpd_i, khat, lppd_i))
    return loo_pit_from_accumulators(*cols, elpd_i, khat, lppd_i, n_draws, pointwise=pointwise)
