"""Pointwise log-likelihood of a trace, streaming WAIC and streaming PSIS-LOO, on the device.

`pm.compute_log_likelihood(idata)` (pymc/stats/log_density.py) evaluates the element-wise log-density of every observed variable at
every draw; `az.waic` reduces that (chains x draws x observations) array per observation.  Here both run on the engine
(csrc/loglik_kernel.h): `compute_log_likelihood` returns the arrays, `waic` accumulates the per-observation reductions on the device
while the draws stream by and never holds the matrix -- the models this engine exists for have 10^6 observations.  `loo` (`az.loo`)
does the same for Pareto-smoothed importance sampling (csrc/psis.h): per observation the tail of the importance ratios and one sum.

The draws are what `sample()` returns: raveled, UNCONSTRAINED positions (chains, draws, n).
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np

from pymc_amd import model_spec as ms


def _spec_of(model):
    from pymc_amd.lowering import as_model_spec

    return as_model_spec(model)


def refusal(spec, nodes=None) -> Optional[str]:
    """Why the pointwise log-likelihood of `spec` (of its observed `nodes`) cannot be computed from the continuous draws alone."""
    if getattr(spec, "extra", None):
        return ("the spec has extra inputs " + repr(sorted(spec.extra)) + ": its likelihood depends on the state another step method "
                "held at each draw, which the continuous draws do not carry")
    for name, kind, _, _ in (ms.observed_nodes(spec) if nodes is None else nodes):
        if kind == ms.LL_MIXTURE and spec.mixture_rows.assign is not None:
            return (f"{name!r} is a conditional mixture: its likelihood depends on the assignments another step method rewrites "
                    "per draw (only the marginal form is supported)")
    return None


def _draws_array(draws, n: int) -> np.ndarray:
    if isinstance(draws, dict):
        draws = draws["draws"]
    a = np.ascontiguousarray(draws, dtype="float64")
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[2] != n:
        raise ValueError(f"draws must be (chains, draws, {n}) raveled unconstrained positions, got {a.shape}")
    return a


def _select(spec, var_names) -> List[Tuple[str, int, int, int]]:
    nodes = ms.observed_nodes(spec)
    if var_names is None:
        return nodes
    if isinstance(var_names, str):
        var_names = [var_names]
    by_name = {nd[0]: nd for nd in nodes}
    missing = [v for v in var_names if v not in by_name]
    if missing:
        raise KeyError(f"not observed variables of the model: {missing} (observed: {sorted(by_name)})")
    return [by_name[v] for v in var_names]


def caller_order(spec, kind: int, values: np.ndarray) -> np.ndarray:
    """Logit rows are evaluated in the spec's group-sorted order: back to the order the observations were passed in."""
    order = getattr(spec, "rows_order", None)
    if kind != ms.LL_LOGIT_ROWS or order is None:
        return values
    out = np.empty_like(values)
    out[..., np.asarray(order)] = values
    return out


def _function(spec, device, func):
    if func is not None:
        return func, False
    from pymc_amd.value_grad import DeviceValueGradFunction

    return DeviceValueGradFunction(spec, device=device), True


def compute_log_likelihood(model, draws, *, var_names=None, device: Optional[int] = None, func=None) -> Dict[str, np.ndarray]:
    """`pm.compute_log_likelihood`: {observed variable: (chains, draws, size)} -- element i of an observed variable at every draw, in
    the order the observations were passed.  A model without observed variables gives {}.  `func`: a `DeviceValueGradFunction` of
    the spec to evaluate on (default: one is built on `device` and closed)."""
    spec = _spec_of(model)
    nodes = _select(spec, var_names)
    why = refusal(spec, nodes)
    if why:
        raise ValueError("log-likelihood refused: " + why)
    if not nodes:
        return {}
    q = _draws_array(draws, spec.n)
    f, own = _function(spec, device, func)
    try:
        out = {}
        for name, kind, index, size in nodes:
            ll = f.log_likelihood(name, q.reshape(-1, spec.n), node=(kind, index))
            out[name] = caller_order(spec, kind, ll).reshape(q.shape[0], q.shape[1], size)
        return out
    finally:
        if own:
            f.close()


def waic_from_accumulators(m, r, mean, m2, n_draws: int, pointwise: bool = False) -> dict:
    """ArviZ's `waic` (log scale) from the four per-observation accumulators of S = `n_draws` pooled draws: m the maximum and
    r = sum exp(ll - m) (lppd_i = log r + m - log S), Welford's mean and M2 (p_waic_i = M2 / S, the population variance)."""
    m, r, m2 = (np.asarray(a, dtype="float64") for a in (m, r, m2))
    S = float(n_draws)
    with np.errstate(divide="ignore", invalid="ignore"):
        lppd_i = np.log(r) + m - np.log(S)
    p_i = m2 / S
    elpd_i = lppd_i - p_i
    N = elpd_i.size
    out = {
        "elpd_waic": float(elpd_i.sum()),
        "se": float(np.sqrt(N * np.var(elpd_i))),
        "p_waic": float(p_i.sum()),
        "lppd": float(lppd_i.sum()),
        "n_samples": int(n_draws),
        "n_data_points": int(N),
        "warning": bool(np.any(p_i > 0.4)),
    }
    if pointwise:
        out["waic_i"] = elpd_i
        out["lppd_i"] = lppd_i
        out["p_waic_i"] = p_i
    return out


def waic(model, draws, *, var_name: Optional[str] = None, pointwise: bool = False, device: Optional[int] = None, func=None) -> dict:
    """`az.waic(idata, var_name=...)` with the chains pooled: elpd_waic, se, p_waic, lppd, n_samples, n_data_points, warning (and
    waic_i with `pointwise`), from accumulators that stay on the device -- the (draws x observations) matrix is never formed."""
    spec = _spec_of(model)
    nodes = ms.observed_nodes(spec)
    why = refusal(spec, [])
    if why:
        raise ValueError("log-likelihood refused: " + why)
    if not nodes:
        raise ValueError("the model has no observed variable")
    if var_name is None and len(nodes) > 1:
        raise TypeError(f"Found several log likelihood arrays {[nd[0] for nd in nodes]}, var_name cannot be None")
    node = _select(spec, var_name)[0]
    why = refusal(spec, [node])
    if why:
        raise ValueError("log-likelihood refused: " + why)
    q = _draws_array(draws, spec.n)
    f, own = _function(spec, device, func)
    try:
        acc = f.waic_accumulator(node[0], node=(node[1], node[2]))
        try:
            for c in range(q.shape[0]):
                acc.update(q[c])
            a, n_draws = acc.raw()
        finally:
            acc.close()
    finally:
        if own:
            f.close()
    a = caller_order(spec, node[1], a)
    return waic_from_accumulators(a[0], a[1], a[2], a[3], n_draws, pointwise=pointwise)


def loo_from_pointwise(elpd_loo_i, khat_i, lppd_i, n_draws: int, pointwise: bool = False) -> dict:
    """ArviZ's `loo` (log scale) from the per-observation results of PSIS over S = `n_draws` pooled draws: elpd_loo = sum elpd_loo_i,
    p_loo = sum lppd_i - elpd_loo, se = sqrt(N var(elpd_loo_i)); `warning` when a Pareto shape exceeds good_k = min(1 - 1 / log10 S, 0.7)."""
    elpd_i, khat, lppd_i = (np.asarray(a, dtype="float64") for a in (elpd_loo_i, khat_i, lppd_i))
    N = elpd_i.size
    good_k = min(1.0 - 1.0 / math.log10(float(n_draws)), 0.7)
    with np.errstate(invalid="ignore"):
        out = {
            "elpd_loo": float(elpd_i.sum()),
            "se": float(np.sqrt(N * np.var(elpd_i))),
            "p_loo": float(lppd_i.sum() - elpd_i.sum()),
            "n_samples": int(n_draws),
            "n_data_points": int(N),
            "warning": bool(np.any(khat > good_k)),
            "good_k": float(good_k),
        }
    if pointwise:
        out["loo_i"] = elpd_i
        out["pareto_k"] = khat
    return out


def loo(model, draws, *, var_name: Optional[str] = None, pointwise: bool = False, reff: float = 1.0, device: Optional[int] = None,
        func=None) -> dict:
    """`az.loo(idata, var_name=...)` with the chains pooled in chain order: elpd_loo, se, p_loo, n_samples, n_data_points, warning,
    good_k (and loo_i, pareto_k with `pointwise`), by Pareto-smoothed importance sampling from a state that stays on the device -- per
    observation the tail of its importance ratios and one running sum; the (draws x observations) matrix is never formed.

    `reff` is the relative efficiency of the draws (ArviZ's `reff` argument; 1.0: no correction).  ArviZ's own default estimates it
    from the autocorrelation of exp(ll) per observation, which needs the whole matrix: that estimate is out of scope here, pass the
    value if you have it."""
    spec = _spec_of(model)
    nodes = ms.observed_nodes(spec)
    why = refusal(spec, [])
    if why:
        raise ValueError("log-likelihood refused: " + why)
    if not nodes:
        raise ValueError("the model has no observed variable")
    if var_name is None and len(nodes) > 1:
        raise TypeError(f"Found several log likelihood arrays {[nd[0] for nd in nodes]}, var_name cannot be None")
    node = _select(spec, var_name)[0]
    why = refusal(spec, [node])
    if why:
        raise ValueError("log-likelihood refused: " + why)
    q = _draws_array(draws, spec.n)
    n_draws = q.shape[0] * q.shape[1]
    f, own = _function(spec, device, func)
    try:
        acc = f.psis_accumulator(node[0], n_draws, reff=reff, node=(node[1], node[2]))
        try:
            for c in range(q.shape[0]):
                acc.update(q[c])
            elpd_i, khat, lppd_i, _ = acc.read()
        finally:
            acc.close()
    finally:
        if own:
            f.close()
    elpd_i, khat, lppd_i = (caller_order(spec, node[1], a) for a in (elpd_i, khat, lppd_i))
    return loo_from_pointwise(elpd_i, khat, lppd_i, n_draws, pointwise=pointwise)
