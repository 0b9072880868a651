"""Power-scaling sensitivity restated in NumPy (no ArviZ here): Kallioinen, Paananen, Buerkner, Vehtari 2023, as pymc_amd/csrc/psens.h
states it.

  * `weights`       the normalised Pareto-smoothed weights of one component at one alpha and their khat: `psis_reference` /
                    `loo_pit_reference.psis_weights` (tied values share the mean weight of their ranks) on the ONE column
                    v = (1 - alpha) lc, divided by their sum;
  * `distance`      D(x, w) in float64, straight from the definition: a stable sort (ties by draw number), numpy.cumsum;
  * `distance_mp`   the same D from the same float64 draws and weights in 200-bit arithmetic (mpmath): the truth;
  * `psens_arrays`  cjs_lo, cjs_hi, sensitivity per parameter; `diagnose` the priorsense table's last column.
"""
import math

import loo_pit_reference as lpr
import mpmath as mp
import numpy as np
import psis_reference as pr

COLUMNS = ("cjs_lo", "cjs_hi", "sensitivity")
MP_BITS = 200


def alphas(delta=0.01):
    return 1.0 / (1.0 + delta), 1.0 + delta


def weights(lc, alpha):
    """(w [S], khat) of one alpha; all NaN when an lc is not finite"""
    lc = np.asarray(lc, dtype="float64").ravel()
    if not np.all(np.isfinite(lc)):
        return np.full(lc.size, np.nan), math.nan
    v = (1.0 - alpha) * lc
    w = lpr.psis_weights(v)
    khat = pr.psis_direct(v)[0]
    return w / w.sum(), float(khat)


def _log2(t):
    out = np.zeros_like(t)
    nz = t != 0.0
    out[nz] = np.log2(t[nz])
    return out


def distance(x, w):
    """D(x, w): NaN for a constant x"""
    x = np.asarray(x, dtype="float64")
    w = np.asarray(w, dtype="float64")
    S = x.size
    order = np.argsort(x, kind="stable")
    xs, ws = x[order], w[order]
    bw = np.diff(xs)
    P = np.arange(1, S, dtype="float64") / S
    Q = np.cumsum(ws)[:-1]
    with np.errstate(all="ignore"):
        M = (P + Q) / 2.0
        Pi, Qi = np.sum(bw * P), np.sum(bw * Q)
        pq = np.sum(bw * P * (_log2(P) - _log2(M))) + (Qi - Pi) / (2.0 * math.log(2.0))
        qp = np.sum(bw * Q * (_log2(Q) - _log2(M))) + (Pi - Qi) / (2.0 * math.log(2.0))
        pq = 0.0 if pq < 0.0 else pq
        qp = 0.0 if qp < 0.0 else qp
        if Pi + Qi == 0.0:
            return math.nan
        return float((pq + qp) / (Pi + Qi))


def distance_mp(x, w):
    """D(x, w) of the same float64 inputs at MP_BITS bits, rounded to float64 at the end"""
    x = np.asarray(x, dtype="float64")
    w = np.asarray(w, dtype="float64")
    S = x.size
    order = np.argsort(x, kind="stable")
    with mp.workprec(MP_BITS):
        xs = [mp.mpf(float(v)) for v in x[order]]
        ws = [mp.mpf(float(v)) for v in w[order]]
        L = lambda t: mp.log(t, 2) if t != 0 else mp.mpf(0)   # noqa: E731
        Pi = Qi = A = B = mp.mpf(0)
        Q = mp.mpf(0)
        for j in range(S - 1):
            Q += ws[j]
            bw = xs[j + 1] - xs[j]
            P = mp.mpf(j + 1) / S
            lm = L((P + Q) / 2)
            Pi += bw * P
            Qi += bw * Q
            A += bw * P * (L(P) - lm)
            B += bw * Q * (L(Q) - lm)
        if Pi + Qi == 0:
            return math.nan
        pq = max(A + (Qi - Pi) / (2 * mp.log(2)), mp.mpf(0))
        qp = max(B + (Pi - Qi) / (2 * mp.log(2)), mp.mpf(0))
        return float((pq + qp) / (Pi + Qi))


def distance_both(x, w, fn=distance):
    """max(D(x, w), D(-x, w)): what cjs_lo^2 / cjs_hi^2 are (NaN if either is)"""
    x = np.asarray(x, dtype="float64")
    a, b = fn(x, w), fn(-x, w)
    return math.nan if math.isnan(a) or math.isnan(b) else max(a, b)


def psens_one(x, w_lo, w_hi, delta=0.01, fn=distance):
    """(D_lo, D_hi, sensitivity) of one parameter; all NaN with a non-finite draw"""
    x = np.asarray(x, dtype="float64")
    if not np.all(np.isfinite(x)):
        return math.nan, math.nan, math.nan
    with np.errstate(all="ignore"):
        d_lo, d_hi = distance_both(x, w_lo, fn), distance_both(x, w_hi, fn)
        return d_lo, d_hi, (math.sqrt(d_lo) + math.sqrt(d_hi)) / (2.0 * math.log2(1.0 + delta))


def psens_arrays(x, lc, delta=0.01):
    """x [S, P], lc [S] -> {cjs_lo, cjs_hi, sensitivity: [P], khat_lo, khat_hi}"""
    x = np.asarray(x, dtype="float64")
    x = x.reshape(x.shape[0], -1)
    a_lo, a_hi = alphas(delta)
    w_lo, k_lo = weights(lc, a_lo)
    w_hi, k_hi = weights(lc, a_hi)
    rows = np.array([psens_one(x[:, p], w_lo, w_hi, delta) for p in range(x.shape[1])]).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return {"cjs_lo": np.sqrt(rows[:, 0]), "cjs_hi": np.sqrt(rows[:, 1]), "sensitivity": rows[:, 2], "khat_lo": k_lo, "khat_hi": k_hi}


def diagnose(prior, likelihood, threshold=0.05):
    out = []
    for p, l in zip(prior, likelihood):
        if math.isnan(p) or math.isnan(l) or not p > threshold:
            out.append("-")
        else:
            out.append("prior-data conflict" if l > threshold else "strong prior / weak likelihood")
    return out
