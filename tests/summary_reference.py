"""The convergence summary of a trace restated in NumPy: every column of `az.summary(kind="all")` as the issue of the device path
defines it (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021), with DIRECT autocovariances (`np.dot` per lag) where
pymc_amd/stats.py takes an FFT.  A plain helper module: tests/test_summary_host.py pins it to stats.py, to tests/golden/stats_kat.npz
and to closed forms and holds pymc_amd/csrc/summary.h to it; tests/test_gpu_summary.py holds the device to it.

For one scalar parameter x[C][N], S = C N:  split(x) is (2 C, N // 2) (the middle draw of an odd N dropped), z(a) =
ndtri((average rank - 3/8) / (size + 1/4)) over all entries of a, ess(a) is stats._ess_raw(a).
"""
import math

import numpy as np
from scipy import special as _sp
from scipy import stats as _st

COLUMNS = ("mean", "sd", "hdi_lo", "hdi_hi", "mcse_mean", "mcse_sd", "ess_bulk", "ess_tail", "r_hat")


def split(x):
    c, n = x.shape
    h = n // 2
    return np.concatenate([x[:, :h], x[:, n - h:]], axis=0)


def z_scale(a):
    r = _st.rankdata(a.ravel(), method="average").reshape(a.shape)
    return _sp.ndtri((r - 0.375) / (a.size + 0.25))


def ess(a):
    """stats._ess_raw line by line, its autocovariance taken by lagged dot products and only at the lags the scan reads"""
    a = np.asarray(a, dtype="float64")
    c, n = a.shape
    if n < 4:
        return float("nan")
    chain_mean = a.mean(axis=1)
    xc = a - chain_mean[:, None]

    def acov(t):   # biased, per chain: (chains,)
        return np.array([np.dot(xc[k, : n - t], xc[k, t:]) for k in range(c)]) / n

    mean_var = acov(0).mean() * n / (n - 1.0)
    var_plus = mean_var * (n - 1.0) / n
    if c > 1:
        var_plus += chain_mean.var(ddof=1)
    if var_plus == 0:
        return float(c * n)
    rho = np.zeros(n)
    rho[0] = 1.0
    rho[1] = 1.0 - (mean_var - acov(1).mean()) / var_plus
    t = 1
    rho_even, rho_odd = 1.0, rho[1]
    while t < n - 3 and (rho_even + rho_odd) > 0:
        rho_even = 1.0 - (mean_var - acov(t + 1).mean()) / var_plus
        rho_odd = 1.0 - (mean_var - acov(t + 2).mean()) / var_plus
        if rho_even + rho_odd >= 0:
            rho[t + 1], rho[t + 2] = rho_even, rho_odd
        t += 2
    max_t = t - 2 if t >= 2 else 0
    if rho_even > 0:
        rho[max_t + 1] = rho_even
    tt = 1
    while tt <= max_t - 2:
        if rho[tt + 1] + rho[tt + 2] > rho[tt - 1] + rho[tt]:
            rho[tt + 1] = (rho[tt - 1] + rho[tt]) / 2.0
            rho[tt + 2] = rho[tt + 1]
        tt += 2
    tau = -1.0 + 2.0 * rho[: max_t + 1].sum() + rho[max_t + 1]
    tau = max(tau, 1.0 / np.log10(c * n))
    return float(c * n / tau)


def rhat_of(zz):
    c, n = zz.shape
    w = zz.var(axis=1, ddof=1).mean()
    b = n * zz.mean(axis=1).var(ddof=1)
    return float(np.sqrt(((n - 1) / n * w + b / n) / w))


def quantile_sorted(xs, q):
    """numpy.quantile's default linear rule on sorted values: its virtual index and `_lerp`, literally"""
    n = len(xs)
    vi = (n - 1) * q
    if vi >= n - 1:
        return float(xs[-1])
    if vi < 0:
        return float(xs[0])
    prev = math.floor(vi)
    t = vi - prev
    a, b = float(xs[prev]), float(xs[prev + 1])
    diff = b - a
    return b - diff * (1 - t) if t >= 0.5 else a + diff * t


def hdi_sorted(xs, hdi_prob):
    S = len(xs)
    k = int(math.floor(hdi_prob * S))
    if S - k < 1:
        return float("nan"), float("nan")
    i = int(np.argmin(xs[k:] - xs[: S - k]))
    return float(xs[i]), float(xs[i + k])


def summarize_one(x, hdi_prob=0.94):
    """{column: float} of x = (chains, draws)"""
    x = np.asarray(x, dtype="float64")
    if x.ndim == 1:
        x = x[None, :]
    out = dict.fromkeys(COLUMNS, float("nan"))
    if not np.all(np.isfinite(x)):
        return out
    with np.errstate(all="ignore"):
        C, N = x.shape
        S = C * N
        mean = float(x.mean())
        d = (x - mean) ** 2
        sd = float(np.sqrt(d.sum() / (S - 1))) if S > 1 else float("nan")
        xs = np.sort(x.ravel())
        out["mean"], out["sd"] = mean, sd
        out["hdi_lo"], out["hdi_hi"] = hdi_sorted(xs, hdi_prob)
        if N // 2 < 1:
            return out
        s = split(x)
        folded = np.abs(s - np.median(s))
        z = z_scale(s)
        out["r_hat"] = max(rhat_of(z), rhat_of(z_scale(folded)))
        out["ess_bulk"] = ess(z)
        q05, q95 = quantile_sorted(xs, 0.05), quantile_sorted(xs, 0.95)
        out["ess_tail"] = min(ess(split((x <= q05).astype("float64"))), ess(split((x <= q95).astype("float64"))))
        out["mcse_mean"] = sd / math.sqrt(ess(s))
        e = ess(split(d))
        ev = float(d.mean())
        out["mcse_sd"] = float(np.sqrt((np.mean(d ** 2) - ev ** 2) / e / ev / 4.0))
    return out


def summarize(x, hdi_prob=0.94):
    """{column: (P,)} of x = (chains, draws, P)"""
    x = np.asarray(x, dtype="float64")
    if x.ndim == 2:
        x = x[:, :, None]
    rows = [summarize_one(x[:, :, p], hdi_prob) for p in range(x.shape[2])]
    return {k: np.array([r[k] for r in rows]) for k in COLUMNS}


# ---- shared inputs of the host and the device tests -------------------------------------------------------------------------------
def ar1(rng, C, N, phi):
    e = rng.standard_normal((C, N))
    x = np.empty((C, N))
    x[:, 0] = e[:, 0] / math.sqrt(1.0 - phi * phi) if abs(phi) < 1 else e[:, 0]
    for i in range(1, N):
        x[:, i] = phi * x[:, i - 1] + e[:, i]
    return x


def kinds(C, N, seed):
    """[(label, (C, N))]: the columns every shape is tried with.  The constant is a dyadic number, so that its sums and means are
    exact in any order and `var_plus == 0` is met on the device as it is here."""
    rng = np.random.default_rng(seed)
    shifted = rng.standard_normal((C, N))
    shifted[C - 1] += 0.8
    with_nan = rng.standard_normal((C, N))
    with_nan[C // 2, N // 3] = np.nan
    with_inf = rng.standard_normal((C, N))
    with_inf[0, N - 1] = np.inf
    return [
        ("iid", rng.standard_normal((C, N))),
        ("ar 0.9", ar1(rng, C, N, 0.9)),
        ("ar -0.5", ar1(rng, C, N, -0.5)),
        ("random walk", np.cumsum(rng.standard_normal((C, N)), axis=1)),
        ("one chain shifted", shifted),
        ("rounded to 0.5", np.round(2.0 * rng.standard_normal((C, N))) / 2.0),
        ("cauchy", rng.standard_cauchy((C, N))),
        ("constant", np.full((C, N), 2.5)),
        ("one nan", with_nan),
        ("one +inf", with_inf),
    ]
