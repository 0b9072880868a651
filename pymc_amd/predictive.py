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

`sample_prior_predictive` / `prior_ppc` (`pm.sample_prior_predictive`) put one step in front of all this: the positions themselves are
drawn from the priors of the free variables, in ancestral order on the device (csrc/prior.h, csrc/prior_kernel.h), and then take the
same path.
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


# ---- predictions at new data -----------------------------------------------------------------------------------------------------------
# `pm.set_data(...)` + `pm.sample_posterior_predictive(..., predictions=True)`: the fitted model at rows it has not seen
# (`model_spec.with_data`), and the held-out log predictive density K-fold and train/test validation rest on.  Per new observation
# the engine folds the conditional mean and variance of the likelihood over the draws in closed form (csrc/predict.h,
# csrc/predict_kernel.h): the predicted probability / mean without the Monte Carlo noise of averaged replicates.
PREDICT_REFUSED_FAMILIES = (ms.D_TRUNCNORMAL, ms.D_POTENTIAL, ms.D_DERIVED)


def predict_refusal(spec, nodes=None) -> Optional[str]:
    """Why conditional moments of `spec`'s observed `nodes` cannot be formed: `loglik.refusal`'s reasons, and the families
    csrc/predict.h has no moments for."""
    why = loglik.refusal(spec, nodes)
    if why:
        return why
    for name, kind, index, _ in (ms.observed_nodes(spec) if nodes is None else nodes):
        if kind == ms.LL_FACTOR and spec.factors[index].dist in PREDICT_REFUSED_FAMILIES:
            return f"{name!r} is a {ms.DIST_NAMES[spec.factors[index].dist]} factor: conditional moments of that family are out of scope"
    return None


def predict_from_accumulators(mean_i, var_between_i, var_within_i, lpd_i, n_draws: int, pointwise: bool = True) -> dict:
    """The predictions from the streamed state of S = `n_draws` pooled draws over M new observations: `mean` the posterior
    predictive mean (the mean over the draws of the conditional mean), `var_between` the population variance over the draws of the
    conditional mean, `var_within` the mean over the draws of the conditional variance, `sd` = sqrt(var_between + var_within) -- the
    law of total variance for the empirical mixture of the draws.  With held-out values (`lpd_i` not None): lpd_i = log mean_s
    p(y_i | theta_s), elpd = sum lpd_i and se = sqrt(M var(lpd_i)), the shape of `loglik.loo`'s result (`lpd_i` is dropped without
    `pointwise`).  NaN and inf are not hidden."""
    mean, vb, vw = (np.asarray(a, dtype="float64") for a in (mean_i, var_between_i, var_within_i))
    M = int(mean.size)
    with np.errstate(invalid="ignore"):
        out = {"mean": mean, "var_between": vb, "var_within": vw, "sd": np.sqrt(vb + vw), "n_samples": int(n_draws), "n_data_points": M}
    if lpd_i is not None:
        lpd = np.asarray(lpd_i, dtype="float64")
        with np.errstate(invalid="ignore"):
            out["elpd"] = float(lpd.sum())
            out["se"] = float(np.sqrt(M * np.var(lpd))) if M else float("nan")
        if pointwise:
            out["lpd_i"] = lpd
    return out


def predict(model, draws, new_data, *, var_name: Optional[str] = None, expected: bool = False, replicates: bool = False, random_seed=0,
            chain_ids=None, pointwise: bool = True, device: Optional[int] = None) -> dict:
    """Predictions of the fitted `model` at new data, streamed: `new_data` = {observed variable: dict of arrays} as
    `model_spec.with_data` takes it (`model_spec.data_inputs(spec)` lists the keys).  One device function is built for the model at
    the new rows and closed; the pooled draws stream by in chain order and the (draws x rows) matrix is never formed.  Returns
    `predict_from_accumulators`'s dict for `var_name` (default: the one variable `new_data` names), arrays in the order the new
    rows were passed; with held-out values (`y` / `observed` given) also lpd_i, elpd and se.

    `expected=True` adds "expected" (chains, draws, M): the conditional mean per draw -- PyMC's `mu` / `p` Deterministic at the
    new rows; credible intervals of the prediction come from it.  `replicates=True` adds "predictions" (chains, draws, M): one
    replicate per draw, what `sample_posterior_predictive` draws for the model at the new rows (its refusals, `random_seed`,
    `chain_ids` and global draw index)."""
    spec = ms.with_data(loglik._spec_of(model), new_data)
    if var_name is None:
        if len(new_data) != 1:
            raise TypeError(f"new_data names {sorted(new_data)}, var_name cannot be None")
        var_name = next(iter(new_data))
    node = loglik._select(spec, var_name)[0]
    why = predict_refusal(spec, [node])
    if why:
        raise ValueError("predictions refused: " + why)
    if replicates:
        _nodes_or_refuse(spec, var_name)
    name, kind, index, size = node
    with_y = name not in spec.predict_no_y
    q = loglik._draws_array(draws, spec.n)
    ids = _chain_ids(draws, chain_ids, q.shape[0])
    f, _ = loglik._function(spec, device, None)
    try:
        acc = f.pred_accumulator(name, with_y=with_y, node=(kind, index))
        try:
            for c in range(q.shape[0]):
                acc.update(q[c])
            mean_i, vb, vw, lpd_i, n_draws = acc.read()
        finally:
            acc.close()
        cols = [loglik.caller_order(spec, kind, a) for a in (mean_i, vb, vw)]
        out = predict_from_accumulators(*cols, loglik.caller_order(spec, kind, lpd_i) if with_y else None, n_draws, pointwise=pointwise)
        if expected:
            e = np.stack([f.predict_moments(name, q[c], node=(kind, index), var=False)[0] for c in range(q.shape[0])])
            out["expected"] = loglik.caller_order(spec, kind, e)
        if replicates:
            y = np.stack([f.posterior_predictive(name, q[k], seed=random_seed, draw0=c * q.shape[1], node=(kind, index)) for k, c in enumerate(ids)])
            out["predictions"] = loglik.caller_order(spec, kind, y)
        return out
    finally:
        f.close()


# ---- prior predictive ----------------------------------------------------------------------------------------------------------------
# `pm.sample_prior_predictive` draws the free variables from their priors, then the data given them.  The first half is the engine's
# `nuts_model_prior` (csrc/prior.h, csrc/prior_kernel.h): S unconstrained positions in ancestral order; the second half is the
# posterior-predictive path above, unchanged, fed with those positions.  `prior_refusal` / `prior_plan` restate the engine's plan
# builder (csrc/engine.hip `prior_build_plan`) on the host, rule by rule and in its order, as `refusal` restates `pp_check`.
PRIOR_INDEX_MAX = 0x3FFF
PRIOR_DISCRETE = (ms.D_BERNOULLI, ms.D_BERNOULLI_LOGIT, ms.D_POISSON)
PRIOR_SAMPLES = 500      # `pm.sample_prior_predictive`'s default number of draws
PRIOR_BATCH = 64         # draws `prior_ppc` asks the engine for at a time (the engine's own batch, csrc/engine.hip PRIOR_B)


def _operands(f, first_arg: int = 0):
    for t in f.args[first_arg:]:
        yield from (t.a, t.b, t.c)
    for ins in (getattr(f, "prog", ()) or ()):
        yield from (ins.x, ins.y, ins.z)


def bare_prior_factors(spec) -> Dict[int, list]:
    """variable -> the factors that are its prior by form: not observed, their value the bare variable, of the variable's size
    (whatever the family: `_prior_analysis` then asks for one it can draw from, `sensitivity` only for a density)."""
    bare: Dict[int, list] = {}
    for fi, f in enumerate(spec.factors):
        t = f.args[0] if f.args else None
        if t is not None and not getattr(f, "observed", False) and t.a.kind == ms.OP_VAR and t.b == ms.ZERO and t.c == ms.ZERO:
            if f.size == spec.vars[t.a.ref].size:
                bare.setdefault(t.a.ref, []).append(fi)
    return bare


def _prior_analysis(spec):
    """-> (why, levels): the reason the prior of `spec` cannot be drawn from (then levels is None), or None and the ancestral order."""
    who = lambda k: f"variable {k} ({spec.vars[k].name!r})"   # noqa: E731
    if spec.mvnormal is not None:
        k = spec.mvnormal.var
        return f"{who(k)} is the MvNormal node's: its prior draw needs a Cholesky factor on the device", None
    mix = getattr(spec, "mixture_rows", None)
    if mix is not None and mix.assign is not None:
        return f"{mix.name!r} is a conditional mixture: its assignments are another step method's", None
    for fi, f in enumerate(spec.factors):
        if f.dist != ms.D_POTENTIAL:
            continue
        for o in _operands(f):
            if o.kind in (ms.OP_VAR, ms.OP_GATHER):
                return f"Potential factor {fi} ({f.name!r}) reads {who(o.ref)}: it reweights the prior", None
            if o.kind == ms.OP_LIN:
                return f"Potential factor {fi} ({f.name!r}) reads a linear predictor: it reweights the prior", None
    prior_of = {}
    bare = bare_prior_factors(spec)
    for k, v in enumerate(spec.vars):
        if k > PRIOR_INDEX_MAX:
            return f"{who(k)}: its index does not fit the 14 bits the counter gives it", None
        over = bare.get(k, [])
        found = [fi for fi in over if spec.factors[fi].dist not in REFUSED_FAMILIES + PRIOR_DISCRETE]
        if not over and mix is not None and mix.w_alpha is not None and mix.w_logits == k and getattr(v, "simplex", False):
            prior_of[k] = -1        # the mixture node's Dirichlet weights: the node owns the prior
            continue
        if not found and over:      # a factor over the bare variable that fails on its family alone
            dist = spec.factors[over[0]].dist
            if dist in REFUSED_FAMILIES:
                return f"{who(k)}: its prior is a {ms.DIST_NAMES[dist]} factor: forward sampling of that family is out of scope", None
            return f"{who(k)}: its prior is a discrete {ms.DIST_NAMES[dist]} factor", None
        if not found:
            return f"{who(k)} has no prior factor (a prior lowered op by op into a program or a Potential cannot be drawn from)", None
        if len(found) > 1:
            return f"{who(k)} has more than one prior factor", None
        f = spec.factors[found[0]]
        if any(o.kind == ms.OP_LIN for o in _operands(f, 1)):
            return f"{who(k)}: its prior reads a linear predictor or a derived vector", None
        prior_of[k] = found[0]
    level: Dict[int, int] = {}
    while len(level) < len(spec.vars):
        new = {}
        for k in range(len(spec.vars)):
            if k in level:
                continue
            parents = set() if prior_of[k] < 0 else {o.ref for o in _operands(spec.factors[prior_of[k]], 1) if o.kind in (ms.OP_VAR, ms.OP_GATHER)}
            if k not in parents and all(p in level for p in parents):
                new[k] = 1 + max((level[p] for p in parents), default=-1)
        if not new:
            return "the priors read each other in a cycle", None
        level.update(new)
    levels = [[] for _ in range(1 + max(level.values(), default=-1))]
    for k, v in enumerate(spec.vars):
        levels[level[k]].append((v.name, prior_of[k]))
    return None, levels


def prior_refusal(spec) -> Optional[str]:
    """Why S positions cannot be drawn from the priors of `spec`'s free variables, or None.  A free variable has a samplable prior
    when exactly one non-observed factor has the bare variable as its value, the variable's size and a continuous family
    `refusal` accepts; the weights of the mixture node under `w ~ Dirichlet` are the node's own."""
    return _prior_analysis(spec)[0]


def prior_plan(spec):
    """The ancestral order of `spec`'s free variables: a list of levels, each a list of (variable name, index of its prior factor;
    -1 for the mixture node's Dirichlet weights).  level(v) = 1 + the largest level of the variables v's prior reads, 0 when it
    reads none.  Raises ValueError where `prior_refusal` gives a reason."""
    why, levels = _prior_analysis(spec)
    if why:
        raise ValueError("prior predictive refused: " + why)
    return levels


def constrained_from_positions(spec, q: np.ndarray) -> Dict[str, np.ndarray]:
    """q (chains, draws, n) -> {name: (chains, draws, *shape)}: the trace's backward transform of the variables (`trace.posterior`)
    and the spec's Deterministics (`trace.deterministics`, what the trace backend records), in that order."""
    from pymc_amd import trace

    out = trace.posterior(spec, q)
    for name, val in trace.deterministics(spec, q.reshape(-1, spec.n)).items():
        out[name] = val.reshape(q.shape[:2] + val.shape[1:])
    return out


def sample_prior_predictive(model, samples: int = PRIOR_SAMPLES, *, var_names=None, random_seed=0, device: Optional[int] = None, func=None) -> dict:
    """`pm.sample_prior_predictive`: `samples` draws of the free variables from their priors, in ancestral order on the device, and one
    replicate of every observed variable at each of them.  Returns

      "q"                  (1, S, n) the raveled UNCONSTRAINED positions -- everything below is a function of them
      "prior"              {variable: (1, S, *constrained shape)}: the trace's backward transform of q, Deterministics included --
                           exactly the values the likelihood kernels saw
      "prior_predictive"   {observed variable: (1, S, size)} = `sample_posterior_predictive(model, q, random_seed=..., chain_ids=[0])`
      "n_nonfinite"        non-finite entries of q (a draw on the boundary of its support, invalid parameters): reported, not hidden

    `random_seed`: the generator's 64-bit key, shared by both halves (their streams never coincide: csrc/prior.h).  `var_names`
    restricts both dicts to the names given.  A model whose observed variables the posterior predictive refuses still gets q and
    prior: the reason is under "prior_predictive_refused" and prior_predictive is {}.  A refused prior raises ValueError."""
    spec = loglik._spec_of(model)
    why = prior_refusal(spec)
    if why:
        raise ValueError("prior predictive refused: " + why)
    S = int(samples)
    if S < 0:
        raise ValueError("samples must not be negative")
    observed = [nd[0] for nd in ms.observed_nodes(spec)]
    names = None if var_names is None else ([var_names] if isinstance(var_names, str) else list(var_names))
    f, own = loglik._function(spec, device, func)
    try:
        q, bad = f.prior(S, seed=random_seed, draw0=0)
        q = q[None]
        prior = constrained_from_positions(spec, q)
        if names is not None:
            missing = [v for v in names if v not in prior and v not in observed]
            if missing:
                raise KeyError(f"not variables of the model: {missing}")
            prior = {k: v for k, v in prior.items() if k in names}
        out = {"q": q, "prior": prior, "prior_predictive": {}, "n_nonfinite": bad}
        wanted = observed if names is None else [v for v in names if v in observed]
        nodes = loglik._select(spec, wanted)
        pp_why = refusal(spec, nodes) if nodes else None
        if pp_why:
            out["prior_predictive_refused"] = pp_why
        elif nodes:
            out["prior_predictive"] = sample_posterior_predictive(spec, q, var_names=wanted, random_seed=random_seed, chain_ids=[0], func=f)
        return out
    finally:
        if own:
            f.close()


def prior_ppc(model, samples: int = PRIOR_SAMPLES, *, var_name: Optional[str] = None, random_seed=0, pointwise: bool = False,
              device: Optional[int] = None, func=None, batch: int = PRIOR_BATCH) -> dict:
    """Streaming prior-predictive checks of one observed variable (see `ppc_from_accumulators`): the positions are drawn from the
    priors `batch` at a time and fed to the accumulators of `ppc`; neither the S positions nor the draws x observations matrix is
    held.  The replicates are those `sample_prior_predictive` returns under the same `random_seed`, whatever `batch` is."""
    spec = loglik._spec_of(model)
    why = prior_refusal(spec)
    if why:
        raise ValueError("prior predictive refused: " + why)
    nodes = ms.observed_nodes(spec)
    why = loglik.refusal(spec, [])
    if why:
        raise ValueError("posterior predictive refused: " + why)
    if not nodes:
        raise ValueError("the model has no observed variable")
    if var_name is None and len(nodes) > 1:
        raise TypeError(f"Found several observed variables {[nd[0] for nd in nodes]}, var_name cannot be None")
    node = _nodes_or_refuse(spec, var_name)[0]
    S, step = int(samples), max(int(batch), 1)
    f, own = loglik._function(spec, device, func)
    try:
        acc = f.ppc_accumulator(node[0], seed=random_seed, node=(node[1], node[2]))
        try:
            for s0 in range(0, S, step):
                acc.update(f.prior(min(step, S - s0), seed=random_seed, draw0=s0)[0])
            mean_i, var_i, n_lt, n_eq, n_draws = acc.read()
            T, T_obs = acc.stats()
        finally:
            acc.close()
    finally:
        if own:
            f.close()
    mean_i, var_i, n_lt, n_eq = (loglik.caller_order(spec, node[1], a) for a in (mean_i, var_i, n_lt, n_eq))
    return ppc_from_accumulators(mean_i, var_i, n_lt, n_eq, T, T_obs, n_draws, pointwise=pointwise)
