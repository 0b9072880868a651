"""NumPy restatement of pymc_amd/csrc/predict.h: the conditional moments of every family (`moments`, `mixture_moments`), the fold of
one observation's per-draw values (`fold`, the recurrences of pd_fold, draw by draw), and `predict` on a given (draws x rows) set of
moments and log-densities -- what `pymc_amd.predictive.predict` returns, computed directly from the matrices.

Argument conventions are those of tests/predictive_reference.py `draw`: (a1, a2, a3) are the factor's arguments 1 .. 3.
"""
import math

import numpy as np

from predictive_reference import (D_BERNOULLI, D_BERNOULLI_LOGIT, D_BETA, D_BINOMIAL, D_CAUCHY, D_DERIVED, D_EXPONENTIAL, D_GAMMA,  # noqa: F401
                                  D_HALFCAUCHY, D_HALFNORMAL, D_INVGAMMA, D_LAPLACE, D_LOGNORMAL, D_NORMAL, D_POISSON, D_POTENTIAL,
                                  D_STUDENTT, D_TRUNCNORMAL, D_UNIFORM)

REFUSED = (D_TRUNCNORMAL, D_POTENTIAL, D_DERIVED)


def sigmoid(x):
    """scalar_math.h sigmoid_d"""
    x = np.asarray(x, dtype="float64")
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def moments(dist, a1, a2=0.0, a3=0.0):
    """-> (mean, var), broadcast over the arguments.  Invalid parameters give NaN for both; a moment that diverges is +inf, one
    that does not exist NaN."""
    if dist in REFUSED or not 0 <= dist <= D_POISSON:
        raise ValueError(f"family {dist} refused: no conditional moments for it")
    a1, a2, a3 = np.broadcast_arrays(*(np.asarray(a, dtype="float64") for a in (a1, a2, a3)))
    nan, inf = np.full(a1.shape, np.nan), np.full(a1.shape, np.inf)
    with np.errstate(all="ignore"):
        if dist == D_NORMAL:
            ok, m, v = a2 > 0, a1, a2 * a2
        elif dist == D_HALFNORMAL:
            ok, m, v = a1 > 0, a1 * 0.79788456080286535588, a1 * a1 * 0.36338022763241865692
        elif dist == D_CAUCHY:
            ok, m, v = a2 > 0, nan, nan
        elif dist == D_HALFCAUCHY:
            ok, m, v = a1 > 0, inf, nan
        elif dist == D_STUDENTT:
            ok = (a1 > 0) & (a3 > 0) & (a1 > 1.0)
            m, v = a2, np.where(a1 > 2.0, a3 * a3 * (a1 / (a1 - 2.0)), np.inf)
        elif dist == D_BETA:
            s = a1 + a2
            ok, m, v = (a1 > 0) & (a2 > 0), a1 / s, a1 * a2 / (s * s * (s + 1.0))
        elif dist == D_EXPONENTIAL:
            ok, m = a1 > 0, 1.0 / a1
            v = m * m
        elif dist == D_UNIFORM:
            w = a2 - a1
            ok, m, v = a1 <= a2, 0.5 * (a1 + a2), w * w / 12.0
        elif dist == D_BERNOULLI_LOGIT:
            ok, m = a1 == a1, sigmoid(a1)
            v = m * sigmoid(-a1)
        elif dist == D_LOGNORMAL:
            s2 = a2 * a2
            ok, m, v = a2 > 0, np.exp(a1 + 0.5 * s2), np.expm1(s2) * np.exp(2.0 * a1 + s2)
        elif dist == D_BERNOULLI:
            ok, m, v = (a1 >= 0) & (a1 <= 1), a1, a1 * (1.0 - a1)
        elif dist == D_BINOMIAL:
            ok, m = (a1 >= 0) & (a2 >= 0) & (a2 <= 1), a1 * a2
            v = m * (1.0 - a2)
        elif dist == D_GAMMA:
            be = 1.0 / (1.0 / a2)
            ok, m = (a1 > 0) & (be > 0), a1 / be
            v = m / be
        elif dist == D_INVGAMMA:
            ok = (a1 > 0) & (a2 > 0)
            m1 = a2 / (a1 - 1.0)
            m = np.where(a1 > 1.0, m1, np.inf)
            v = np.where(a1 > 1.0, np.where(a1 > 2.0, m1 * m1 / (a1 - 2.0), np.inf), np.nan)
        elif dist == D_LAPLACE:
            ok, m, v = a2 > 0, a1, 2.0 * a2 * a2
        else:  # D_POISSON
            ok, m, v = a1 >= 0, a1, a1
        return np.where(ok, m, np.nan), np.where(ok, v, np.nan)


def mixture_moments(mu, sigma, w):
    """pd_mixture: sums in index order; mu, sigma, w [..., K] -> (mean [...], var [...])"""
    mu, sigma, w = (np.asarray(a, dtype="float64") for a in (mu, sigma, w))
    K = mu.shape[-1]
    m = np.zeros(np.broadcast(mu, w).shape[:-1])
    for k in range(K):
        m = m + w[..., k] * mu[..., k]
    v = np.zeros_like(m)
    for k in range(K):
        d = mu[..., k] - m
        v = v + w[..., k] * (sigma[..., k] * sigma[..., k] + d * d)
    return m, v


def _run_mean(mean, x, k):
    """pd_run_mean, element-wise"""
    with np.errstate(all="ignore"):
        plain = mean + (x - mean) / k
    nan = np.isnan(x) | np.isnan(mean)
    xi, mi = np.isinf(x), np.isinf(mean)
    out = np.where(xi, x, plain)
    out = np.where(mi, mean, out)
    out = np.where(xi & mi & (x != mean), np.nan, out)
    return np.where(nan, np.nan, out)


def fold(m, v, lp=None, state=None):
    """pd_fold over the rows of m, v (and lp) [S, N], in order -> the state (mean, M2, vbar, lmax, lsum, count), each [N]; `state`
    continues an earlier fold."""
    m, v = np.asarray(m, dtype="float64"), np.asarray(v, dtype="float64")
    N = m.shape[1]
    if state is None:
        state = (np.zeros(N), np.zeros(N), np.zeros(N), np.full(N, -np.inf), np.zeros(N), 0.0)
    mean, M2, vbar, lmax, lsum = (np.array(a, dtype="float64") for a in state[:5])
    count = float(state[5])
    with np.errstate(all="ignore"):
        for s in range(m.shape[0]):
            count += 1.0
            dl = m[s] - mean
            mean = _run_mean(mean, m[s], count)
            M2 = M2 + dl * (m[s] - mean)
            vbar = _run_mean(vbar, v[s], count)
            if lp is not None:
                x = np.asarray(lp[s], dtype="float64")
                up = x > lmax
                scaled = np.where(lmax == -np.inf, 0.0, lsum * np.exp(lmax - x)) + 1.0
                add = lsum + np.where(x == lmax, 1.0, np.exp(x - lmax))
                new = np.where(up, scaled, np.where(x > -np.inf, add, np.where(np.isnan(x), x, lsum)))
                lmax = np.where(up, x, lmax)
                lsum = new
    return mean, M2, vbar, lmax, lsum, count


def read(state, with_lp=True):
    """nuts_pred_read: (mean_i, var_between_i, var_within_i, lpd_i or None)"""
    mean, M2, vbar, lmax, lsum, count = state
    with np.errstate(all="ignore"):
        lpd = np.log(lsum) + lmax - math.log(count) if with_lp else None
        return mean, M2 / count, vbar, lpd


def predict(m, v, lp=None):
    """`predictive.predict`'s dict from the matrices m, v (and lp) [S, M], directly: population variance, logsumexp - log S."""
    from scipy.special import logsumexp

    m, v = np.asarray(m, dtype="float64"), np.asarray(v, dtype="float64")
    S, M = m.shape
    with np.errstate(all="ignore"):
        out = {"mean": m.mean(axis=0), "var_between": m.var(axis=0), "var_within": v.mean(axis=0), "n_samples": S, "n_data_points": M}
        out["sd"] = np.sqrt(out["var_between"] + out["var_within"])
        if lp is not None:
            lpd = logsumexp(np.asarray(lp, dtype="float64"), axis=0) - math.log(S)
            out.update({"lpd_i": lpd, "elpd": float(lpd.sum()), "se": float(np.sqrt(M * np.var(lpd)))})
    return out
