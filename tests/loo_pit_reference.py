"""LOO-PIT and the LOO predictive moments restated in NumPy on whole vectors (no ArviZ here).

Per observation, from its S log-likelihood values `ll` and S replicates `y_rep`:
  * `psis_weights`  the normalised Pareto-smoothed weights of `psis_reference.psis_direct` (ArviZ's `psislw`), with ONE deliberate
                    difference: draws of the tail whose values are tied share the arithmetic mean of the weights of the ranks they
                    occupy.  ArviZ hands tied values different weights in the order the draws are stored (a stable argsort), so its
                    LOO-PIT changes when the trace is permuted; the mean keeps sum w = 1, does not depend on the order and is
                    ArviZ's whenever no value repeats (`psis_weights(..., tie_mean=False)` is the argsort rule).
  * `loo_pit_vector`  p_lt = sum w [y_rep < y], p_eq = sum w [y_rep == y] (ArviZ's `loo_pit` is p_lt + p_eq), the weighted mean and
                    population variance of y_rep, ess = 1 / sum w^2.
A NaN or +inf value (poisoned) or a -inf value (degenerate: elpd = -inf) gives NaN for everything, the engine's convention.
"""
import math

import numpy as np
import psis_reference as pr

COLUMNS = ("p_lt", "p_eq", "loo_mean", "loo_sd", "ess", "sum_w")


def psis_weights(ll, reff=1.0, tie_mean=True):
    """The S normalised weights of one observation; all NaN for a degenerate or poisoned vector."""
    ll = np.asarray(ll, dtype="float64")
    if pr._special(ll):
        return np.full(ll.size, np.nan)
    S = ll.size
    M = pr.tail_len(S, reff)
    x = -ll
    x = x - np.max(x)
    xc = max(np.sort(x)[S - M - 1], pr.LOG_DBL_MIN)
    exc = math.exp(xc)
    tail = np.where(x > xc)[0]
    tl = tail.size
    if tl > 4:
        order = tail[np.argsort(x[tail], kind="stable")]
        khat, sigma = pr.gpdfit(np.exp(x[order]) - exc)
        if math.isfinite(khat):
            with np.errstate(all="ignore"):
                sm = np.log(pr.gpinv((np.arange(tl) + 0.5) / tl, khat, sigma) + exc)
            x = x.copy()
            x[order] = np.minimum(sm, 0.0)
    w = np.exp(x - pr._lse(x))
    if tie_mean and tl:
        vals, inverse, counts = np.unique(ll[tail], return_inverse=True, return_counts=True)
        if np.any(counts > 1):
            sums = np.zeros(vals.size)
            np.add.at(sums, inverse, w[tail])
            w = w.copy()
            w[tail] = (sums / counts)[inverse]
    return w


def loo_pit_vector(ll, y_rep, y, reff=1.0, tie_mean=True):
    """{p_lt, p_eq, loo_mean, loo_sd, ess, sum_w} of one observation"""
    w = psis_weights(ll, reff, tie_mean)
    y_rep = np.asarray(y_rep, dtype="float64")
    if np.any(np.isnan(w)):
        return {k: math.nan for k in COLUMNS}
    W = float(np.sum(w))
    with np.errstate(invalid="ignore"):
        mean = float(np.sum(w * y_rep) / W)
        var = float(np.sum(w * (y_rep - mean) ** 2) / W)
    return {
        "p_lt": float(np.sum(w[y_rep < y])),
        "p_eq": float(np.sum(w[y_rep == y])),
        "loo_mean": mean,
        "loo_sd": math.sqrt(var) if var == var else math.nan,
        "ess": 1.0 / float(np.sum(w * w)),
        "sum_w": W,
    }


def loo_pit_matrix(ll, y_rep, y, reff=1.0, tie_mean=True):
    """{column: [N]} of [S][N] matrices of values and replicates and the N observed values"""
    ll, y_rep, y = np.asarray(ll, dtype="float64"), np.asarray(y_rep, dtype="float64"), np.asarray(y, dtype="float64").ravel()
    rows = [loo_pit_vector(ll[:, i], y_rep[:, i], y[i], reff, tie_mean) for i in range(ll.shape[1])]
    return {k: np.array([r[k] for r in rows]) for k in COLUMNS}
