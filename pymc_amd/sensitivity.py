"""Power-scaling sensitivity of a trace on the device: `az.psens` and the `priorsense` table (Kallioinen, Paananen, Buerkner, Vehtari
2023, "Detecting and diagnosing prior and likelihood sensitivity with power-scaling").  Do the priors matter for this posterior, and
do they fight the data?

One component of the model -- the prior or the likelihood -- is raised to the powers 1 / (1 + delta) and 1 + delta.  The draws are
not sampled again: they are reweighted by Pareto-smoothed importance weights of (alpha - 1) x the component's log-density, and the
sensitivity of a parameter is the cumulative Jensen-Shannon distance between its draws' ECDF and the weighted one, per unit of
log2(alpha).  The definitions are in pymc_amd/csrc/psens.h and DESIGN.md 4.23; the three device calls are `nuts_model_logdens_sum`
(a draw's log-prior / log-likelihood as ONE number, reduced where the pointwise values lie: the draws x observations matrix never
reaches the host), `nuts_psens_weights` and `nuts_psens` (include/nuts_mi355.h).  There is no host fallback.

The draws are what `sample()` returns: raveled, UNCONSTRAINED positions (chains, draws, n); sensitivities are taken over the
CONSTRAINED values of the variables and the Deterministics, as ArviZ works on the posterior group.  The log-prior is the sum of the
prior factors' terms at the constrained values, WITHOUT the Jacobians of the transforms, as `pm.compute_log_prior` gives it.
"""

from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Tuple

import numpy as np

from pymc_amd import _lib, loglik
from pymc_amd import model_spec as ms
from pymc_amd.predictive import _operands, bare_prior_factors, constrained_from_positions
from pymc_amd.summary import flat_names

COLUMNS = ("cjs_lo", "cjs_hi", "sensitivity")
COMPONENTS = ("prior", "likelihood")
THRESHOLD = 0.05         # priorsense's
NOT_A_PRIOR = (ms.D_POTENTIAL, ms.D_DERIVED)


def max_draws() -> int:
    """The largest chains x draws `psens` accepts (one workgroup sorts a parameter's draws in LDS)."""
    return int(_lib.load().nuts_summary_max_draws())


# ---- which factor is a variable's prior ------------------------------------------------------------------------------------------------
def _prior_factors_or_why(spec, names=None) -> Tuple[Optional[str], List[Tuple[str, int]]]:
    who = lambda k: f"variable {k} ({spec.vars[k].name!r})"   # noqa: E731
    for fi, f in enumerate(spec.factors):
        if f.dist != ms.D_POTENTIAL:
            continue
        for o in _operands(f):
            if o.kind in (ms.OP_VAR, ms.OP_GATHER, ms.OP_LIN):
                what = "a linear predictor" if o.kind == ms.OP_LIN else who(o.ref)
                return (f"Potential factor {fi} ({f.name!r}) reads {what}: PyMC leaves Potentials out of compute_log_prior, so scaling "
                        "the prior factors alone would mis-scale this model's prior"), []
    if spec.mvnormal is not None:
        return f"{who(spec.mvnormal.var)} is the MvNormal node's: its prior is not an element-wise factor", []
    mix = getattr(spec, "mixture_rows", None)
    bare = bare_prior_factors(spec)
    out = []
    for k, v in enumerate(spec.vars):
        if names is not None and v.name not in names:
            continue
        found = [fi for fi in bare.get(k, ()) if spec.factors[fi].dist not in NOT_A_PRIOR]
        if not found and mix is not None and mix.w_alpha is not None and mix.w_logits == k:
            return f"{who(k)} holds the mixture node's Dirichlet weights: the node owns their prior (and its transform's Jacobian)", []
        if not found:
            return f"{who(k)} has no prior factor (a prior lowered op by op into a program or a Potential has no density of its own)", []
        if len(found) > 1:
            return f"{who(k)} has more than one prior factor", []
        out.append((v.name, found[0]))
    return None, out


def prior_refusal(spec) -> Optional[str]:
    """Why the log-prior of `spec` cannot be formed from its factors, or None.  A free variable's prior is the one non-observed
    factor whose value is the bare variable and whose size is the variable's (`predictive.bare_prior_factors`), of any family."""
    return _prior_factors_or_why(spec)[0]


def prior_factors(spec, var_names=None) -> List[Tuple[str, int]]:
    """[(variable, index of its prior factor)] in the spec's order; raises ValueError where `prior_refusal` gives a reason."""
    if var_names is not None:
        var_names = [var_names] if isinstance(var_names, str) else list(var_names)
        missing = [v for v in var_names if v not in {u.name for u in spec.vars}]
        if missing:
            raise KeyError(f"not free variables of the model: {missing}")
    why, out = _prior_factors_or_why(spec, var_names)
    if why:
        raise ValueError("log-prior refused: " + why)
    return out


def likelihood_refusal(spec) -> Optional[str]:
    """Why the log-likelihood total cannot be formed: `loglik.refusal`'s reasons, or a model without observed variables."""
    why = loglik.refusal(spec)
    if why:
        return why
    return None if ms.observed_nodes(spec) else "the model has no observed variable"


# ---- log-densities -----------------------------------------------------------------------------------------------------------------------
def compute_log_prior(model, draws, var_names=None, *, device: Optional[int] = None, func=None) -> Dict[str, np.ndarray]:
    """`pm.compute_log_prior`: {variable: (chains, draws, size)} -- the prior factor's term of every element at the constrained value,
    without the transform's Jacobian.  Pointwise, through `nuts_model_loglik` on each variable's prior factor: the small,
    matrix-holding counterpart of `loglik.compute_log_likelihood`."""
    spec = loglik._spec_of(model)
    pf = prior_factors(spec, var_names)
    q = loglik._draws_array(draws, spec.n)
    f, own = loglik._function(spec, device, func)
    try:
        return {name: f.log_likelihood(name, q.reshape(-1, spec.n), node=(ms.LL_FACTOR, fi)).reshape(q.shape[0], q.shape[1], -1) for name, fi in pf}
    finally:
        if own:
            f.close()


def _totals(spec, q, nodes, device, func) -> np.ndarray:
    f, own = loglik._function(spec, device, func)
    try:
        total = np.zeros(q.shape[0] * q.shape[1])
        for kind, index in nodes:       # (in spec order; the first term is added to +0.0)
            total = total + f.logdens_sum(q.reshape(-1, spec.n), (kind, index))
        return total.reshape(q.shape[:2])
    finally:
        if own:
            f.close()


def log_prior(model, draws, *, device: Optional[int] = None, func=None) -> np.ndarray:
    """(chains, draws): the log-prior of every draw as one number -- each prior factor's total from `nuts_model_logdens_sum`, the
    factors added in spec order."""
    spec = loglik._spec_of(model)
    pf = prior_factors(spec)
    return _totals(spec, loglik._draws_array(draws, spec.n), [(ms.LL_FACTOR, fi) for _, fi in pf], device, func)


def log_likelihood(model, draws, *, device: Optional[int] = None, func=None) -> np.ndarray:
    """(chains, draws): the log-likelihood of every draw as one number, over all observed nodes and observations, the nodes added in
    spec order; the pointwise matrix stays on the device."""
    spec = loglik._spec_of(model)
    why = likelihood_refusal(spec)
    if why:
        raise ValueError("log-likelihood refused: " + why)
    return _totals(spec, loglik._draws_array(draws, spec.n), [(nd[1], nd[2]) for nd in ms.observed_nodes(spec)], device, func)


# ---- weights and distances -----------------------------------------------------------------------------------------------------------------
def psens_weights(lc, alpha: float, device: Optional[int] = None) -> Tuple[np.ndarray, float]:
    """(w [S], khat): the normalised Pareto-smoothed weights of scaling a component with log-density `lc` (any shape, pooled in
    storage order) by the power `alpha` (`nuts_psens_weights`)."""
    lc = np.ascontiguousarray(np.asarray(lc, dtype="float64").ravel())
    lib = _lib.load()
    if device is not None:
        _lib.check(lib.nuts_set_device(int(device)), "nuts_set_device")
    w = np.empty(lc.size)
    khat = C.c_double()
    _lib.check(lib.nuts_psens_weights(_lib.dptr(lc), lc.size, float(alpha), _lib.dptr(w), C.byref(khat)), "nuts_psens_weights")
    return w, float(khat.value)


def psens_from_weights(x, w_lo, w_hi, delta: float = 0.01, device: Optional[int] = None) -> Dict[str, np.ndarray]:
    """x (S, P) or (S,) with the weights of the two alphas -> {column: (P,)} (`nuts_psens`)."""
    x = np.asarray(x, dtype="float64")
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2:
        raise ValueError(f"psens: draws of shape (S, P) or (S,), not {x.shape}")
    S, P = x.shape
    w_lo, w_hi = (np.ascontiguousarray(np.asarray(w, dtype="float64").ravel()) for w in (w_lo, w_hi))
    if w_lo.size != S or w_hi.size != S:
        raise ValueError(f"psens: {S} draws, but {w_lo.size} and {w_hi.size} weights")
    lib = _lib.load()
    if device is not None:
        _lib.check(lib.nuts_set_device(int(device)), "nuts_set_device")
    _lib.sync_options_from_env()
    x = np.ascontiguousarray(x)
    out = np.empty((len(COLUMNS), P))
    _lib.check(lib.nuts_psens(_lib.dptr(x), S, P, _lib.dptr(w_lo), _lib.dptr(w_hi), float(delta), _lib.dptr(out)), "nuts_psens")
    return {name: out[k].copy() for k, name in enumerate(COLUMNS)}


def psens_from_arrays(x, lc, delta: float = 0.01, device: Optional[int] = None) -> dict:
    """For callers with their own arrays, no model: x (chains, draws, P) or (S, P) draws of P parameters, lc (chains, draws) or (S,)
    the component's log-density at each draw -> {cjs_lo, cjs_hi, sensitivity: (P,), khat_lo, khat_hi}."""
    x = np.asarray(x, dtype="float64")
    lc = np.asarray(lc, dtype="float64")
    if x.ndim == lc.ndim:
        x = x[..., None]
    if x.shape[:-1] != lc.shape:
        raise ValueError(f"psens: draws of shape {x.shape} do not go with log-densities of shape {lc.shape}")
    if not float(delta) > 0.0:
        raise ValueError(f"psens: delta must be positive, not {delta}")
    x = x.reshape(-1, x.shape[-1])
    S = x.shape[0]
    if S < 2:
        raise ValueError("psens: at least 2 draws")
    if S > max_draws():
        raise ValueError(f"psens: {S} draws per parameter exceed the limit of {max_draws()} (one workgroup sorts a parameter's "
                         "draws in LDS); a larger trace is out of scope")
    w_lo, k_lo = psens_weights(lc, 1.0 / (1.0 + float(delta)), device)
    w_hi, k_hi = psens_weights(lc, 1.0 + float(delta), device)
    out = psens_from_weights(x, w_lo, w_hi, delta, device) if x.shape[1] else {c: np.empty(0) for c in COLUMNS}
    out.update({"khat_lo": k_lo, "khat_hi": k_hi})
    return out


def _constrained(spec, q, var_names):
    post = constrained_from_positions(spec, q)
    if var_names is not None:
        var_names = [var_names] if isinstance(var_names, str) else list(var_names)
        missing = [v for v in var_names if v not in post]
        if missing:
            raise KeyError(f"psens: no variable named {missing} (the model has {list(post)})")
        post = {k: post[k] for k in post if k in set(var_names)}
    names: List[str] = []
    blocks = []
    for name, a in post.items():
        names += flat_names(name, a.shape[2:])
        blocks.append(np.asarray(a, dtype="float64").reshape(a.shape[0], a.shape[1], -1))
    x = np.concatenate(blocks, axis=2) if blocks else np.empty(q.shape[:2] + (0,))
    return names, x


def psens(model, draws, component: str = "prior", delta: float = 0.01, var_names=None, *, device: Optional[int] = None, func=None) -> dict:
    """`az.psens(idata, component=...)`: {"names": rows labelled as `summary.summary` labels them, "cjs_lo", "cjs_hi", "sensitivity":
    (rows,), "khat_lo", "khat_hi": the Pareto shapes of the two sets of weights}.  Raises ValueError where the component is refused
    (`prior_refusal`, `likelihood_refusal`)."""
    if component not in COMPONENTS:
        raise ValueError(f"psens: component must be one of {COMPONENTS}, not {component!r}")
    spec = loglik._spec_of(model)
    q = loglik._draws_array(draws, spec.n)
    names, x = _constrained(spec, q, var_names)
    lc = (log_prior if component == "prior" else log_likelihood)(spec, q, device=device, func=func)
    return {"names": names, **psens_from_arrays(x, lc, delta, device)}


def diagnose(prior, likelihood, threshold: float = THRESHOLD) -> List[str]:
    """priorsense's diagnosis per row: both sensitivities above the threshold: "prior-data conflict"; the prior's alone:
    "strong prior / weak likelihood"; otherwise, and with a NaN in either, "-"."""
    out = []
    for p, l in zip(np.asarray(prior, dtype="float64").ravel(), np.asarray(likelihood, dtype="float64").ravel()):
        if math.isnan(p) or math.isnan(l) or not p > threshold:
            out.append("-")
        else:
            out.append("prior-data conflict" if l > threshold else "strong prior / weak likelihood")
    return out


def psens_table(model, draws, delta: float = 0.01, var_names=None, *, device: Optional[int] = None, func=None) -> dict:
    """The `priorsense` table: {"names", "prior", "likelihood": the sensitivities (rows,), "diagnosis": [str], "prior_khat",
    "likelihood_khat": (khat_lo, khat_hi), "refused": {component: reason}}.  A model for which one component is refused still gets
    the other: the refused one's column is NaN (its rows are diagnosed "-") and the reason is under "refused"."""
    spec = loglik._spec_of(model)
    q = loglik._draws_array(draws, spec.n)
    names, x = _constrained(spec, q, var_names)
    whys = {"prior": prior_refusal(spec), "likelihood": likelihood_refusal(spec)}
    f, own = (None, False) if all(whys.values()) else loglik._function(spec, device, func)
    out = {"names": names, "refused": {}}
    try:
        for comp in COMPONENTS:
            why = whys[comp]
            if why:
                out["refused"][comp] = why
                out[comp] = np.full(len(names), np.nan)
                out[comp + "_khat"] = (math.nan, math.nan)
                continue
            lc = (log_prior if comp == "prior" else log_likelihood)(spec, q, device=device, func=f)
            r = psens_from_arrays(x, lc, delta, device)
            out[comp] = r["sensitivity"]
            out[comp + "_khat"] = (r["khat_lo"], r["khat_hi"])
    finally:
        if own:
            f.close()
    out["diagnosis"] = diagnose(out["prior"], out["likelihood"])
    return out
