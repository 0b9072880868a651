"""Convergence summary of a trace on the device: what `az.summary(idata, kind="all")` prints -- mean, sd, HDI, MCSE of the mean and
of the sd, bulk and tail ESS, R-hat -- for every parameter at once (include/nuts_mi355.h `nuts_summary`; the estimators are stated
in pymc_amd/csrc/summary.h and DESIGN.md 4.19; Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021).

`summarize` takes an array of draws, `summary` a model and the result of `sample` and labels the rows as ArviZ does (`tau`,
`theta[3]`, `L[1, 0]`); `sample(..., summary=True)` attaches the latter to its result.  One workgroup per parameter sorts its draws
in LDS, so chains x draws is limited to `max_draws()`; there is no host fallback (pymc_amd/stats.py stays the benchmark's metric).
"""

from __future__ import annotations

import itertools
from typing import Dict, List, Optional

import numpy as np

from pymc_amd import _lib

COLUMNS = ("mean", "sd", "hdi_lo", "hdi_hi", "mcse_mean", "mcse_sd", "ess_bulk", "ess_tail", "r_hat")


def max_draws() -> int:
    """The largest chains x draws of one parameter `summarize` accepts."""
    return int(_lib.load().nuts_summary_max_draws())


def summarize(x, hdi_prob: float = 0.94, device: Optional[int] = None) -> Dict[str, np.ndarray]:
    """x (chains, draws, P) or (chains, draws) -> {column: (P,)}, the columns of `COLUMNS`.  A parameter with a non-finite draw has
    NaN in every column; with fewer than 4 draws per half chain the ESS and MCSE columns are NaN."""
    x = np.asarray(x, dtype="float64")
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3:
        raise ValueError(f"summarize: draws of shape (chains, draws, P) or (chains, draws), not {x.shape}")
    C, N, P = x.shape
    if C < 1 or N < 1:
        raise ValueError(f"summarize: at least one chain and one draw, not {C} x {N}")
    if not 0.0 < float(hdi_prob) < 1.0:
        raise ValueError(f"summarize: hdi_prob must lie inside (0, 1), not {hdi_prob}")
    lib = _lib.load()
    limit = int(lib.nuts_summary_max_draws())
    if C * N > limit:
        raise ValueError(f"summarize: {C} chains x {N} draws = {C * N} draws per parameter exceed the limit of {limit} "
                         "(one workgroup sorts a parameter's draws in LDS); a larger trace is out of scope")
    if device is not None:
        _lib.check(lib.nuts_set_device(int(device)), "nuts_set_device")
    _lib.sync_options_from_env()
    x = np.ascontiguousarray(x)
    out = np.empty((len(COLUMNS), P))
    _lib.check(lib.nuts_summary(_lib.dptr(x), C, N, P, float(hdi_prob), _lib.dptr(out)), "nuts_summary")
    return {name: out[k].copy() for k, name in enumerate(COLUMNS)}


def flat_names(name: str, shape) -> List[str]:
    """The row labels of one variable as ArviZ writes them: `tau`, `theta[3]`, `L[1, 0]`."""
    shape = tuple(int(s) for s in shape)
    if not shape:
        return [name]
    return [f"{name}[{', '.join(str(i) for i in idx)}]" for idx in itertools.product(*(range(s) for s in shape))]


def summary(model, result_or_draws, var_names=None, include_transformed: bool = False, hdi_prob: float = 0.94, device: Optional[int] = None) -> dict:
    """`az.summary` of the result of `sample` (or of its (chains, draws, n) array of raveled unconstrained draws): the constrained
    value of every variable (`trace.posterior`; with `include_transformed` the value variables as well), flattened to one row per
    element in the model's order, optionally only `var_names`.  Returns {"names": [...], column: (rows,), ...}."""
    from pymc_amd.lowering import as_model_spec
    from pymc_amd.trace import posterior

    spec = as_model_spec(model)
    draws = result_or_draws["draws"] if isinstance(result_or_draws, dict) else result_or_draws
    draws = np.asarray(draws, dtype="float64")
    if draws.ndim != 3 or draws.shape[2] != spec.n:
        raise ValueError(f"summary: draws of shape (chains, draws, {spec.n}) -- the raveled unconstrained positions --, not {draws.shape}")
    post = posterior(spec, draws, include_transformed)
    if var_names is not None:
        missing = [v for v in var_names if v not in post]
        if missing:
            raise KeyError(f"summary: no variable named {missing} (the model has {list(post)})")
        post = {k: post[k] for k in post if k in set(var_names)}
    names: List[str] = []
    blocks = []
    for name, a in post.items():
        names += flat_names(name, a.shape[2:])
        blocks.append(a.reshape(a.shape[0], a.shape[1], -1))
    x = np.concatenate(blocks, axis=2) if blocks else np.empty(draws.shape[:2] + (0,))
    return {"names": names, **summarize(x, hdi_prob, device)}
