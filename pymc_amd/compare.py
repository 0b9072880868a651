"""Model comparison on the device: what `az.compare` reports on the log scale -- the elpd of every model with its standard error, the
difference to the best model with the standard error of that difference, and the model weights by stacking (ArviZ's default),
by pseudo-BMA with the Bayesian bootstrap, or by plain pseudo-BMA (include/nuts_mi355.h `nuts_compare_*`; the definitions, the
bootstrap's counter layout and the stacking solver are stated in pymc_amd/csrc/compare.h and DESIGN.md 4.21; Yao, Vehtari, Simpson,
Gelman 2018).

`compare_pointwise` takes the pointwise elpd of every model, `compare` models with their draws and runs `loglik.loo` or
`loglik.waic` per model first.  The bootstrap's [b_samples][N] weight matrix never exists: its entries come from a counter-based
generator and are recomputed where they are used.  There is no host fallback.
"""

from __future__ import annotations

import ctypes as C
import warnings
from typing import Dict, Optional

import numpy as np

from pymc_amd import _lib

METHODS = ("stacking", "BB-pseudo-BMA", "pseudo-BMA")
MAX_MODELS = 8
MAX_PASSES = 64
GAP_TOL = 1e-10


class Comparison:
    """K models over N observations on the device (`nuts_compare`).  `set(k, elpd_i, order)` uploads a row -- with `order`,
    elpd_i[j] belongs to observation order[j] --; `moments`, `stacking` and `bb` need every row set."""

    def __init__(self, N: int, K: int, device: Optional[int] = None):
        lib = _lib.load()
        if device is not None:
            _lib.check(lib.nuts_set_device(int(device)), "nuts_set_device")
        self._lib = lib
        self.N, self.K = int(N), int(K)
        self._h = lib.nuts_compare_create(self.N, self.K)
        if not self._h:
            msg = _lib.last_error()
            if "no HIP device" in msg or "memory" in msg:
                raise _lib.EngineError(msg)
            raise ValueError(msg)

    def set(self, k: int, elpd_i, order=None) -> None:
        a = np.ascontiguousarray(elpd_i, dtype="float64")
        if a.shape != (self.N,):
            raise ValueError(f"compare: row {k} has shape {a.shape}, not ({self.N},)")
        o = None
        if order is not None:
            o = np.ascontiguousarray(order, dtype="int64")
            if o.shape != (self.N,):
                raise ValueError(f"compare: order has shape {o.shape}, not ({self.N},)")
        _lib.check(self._lib.nuts_compare_set(self._h, int(k), _lib.dptr(a), None if o is None else o.ctypes.data_as(C.POINTER(C.c_int64))),
                   "nuts_compare_set")

    def moments(self):
        """-> elpd [K], se [K], dse [K], best"""
        _lib.sync_options_from_env()
        elpd, se, dse = np.empty(self.K), np.empty(self.K), np.empty(self.K)
        best = C.c_int32(-1)
        _lib.check(self._lib.nuts_compare_moments(self._h, _lib.dptr(elpd), _lib.dptr(se), _lib.dptr(dse), C.byref(best)), "nuts_compare_moments")
        return elpd, se, dse, int(best.value)

    def stacking(self):
        """-> weights [K], objective, kkt_gap, passes"""
        _lib.sync_options_from_env()
        w = np.empty(self.K)
        f, gap, passes = C.c_double(), C.c_double(), C.c_int32()
        _lib.check(self._lib.nuts_compare_stacking(self._h, _lib.dptr(w), C.byref(f), C.byref(gap), C.byref(passes)), "nuts_compare_stacking")
        return w, float(f.value), float(gap.value), int(passes.value)

    def bb(self, b_samples: int = 1000, seed: int = 0, return_z: bool = False):
        """-> weights [K], se_bb [K] (and z [b_samples][K] with `return_z`)"""
        _lib.sync_options_from_env()
        b_samples = int(b_samples)
        w, se = np.empty(self.K), np.empty(self.K)
        z = np.empty((max(b_samples, 0), self.K)) if return_z else None
        _lib.check(self._lib.nuts_compare_bb(self._h, b_samples, int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.dptr(w), _lib.dptr(se),
                                             None if z is None else _lib.dptr(z)), "nuts_compare_bb")
        return (w, se, z) if return_z else (w, se)

    def close(self) -> None:
        if self._h:
            self._lib.nuts_compare_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def pseudo_bma_weights(elpd) -> np.ndarray:
    elpd = np.asarray(elpd, dtype="float64")
    u = np.exp(elpd - elpd.max())
    return u / u.sum()


def cap_warning(gap: float, passes: int, N: int) -> Optional[str]:
    """The text of the warning when the stacking solver stopped at its cap of passes short of its tolerance, else None."""
    if gap > GAP_TOL and passes >= MAX_PASSES:
        return (f"compare: stacking stopped at its cap of {MAX_PASSES} passes with kkt_gap = {gap:.3g} (> {GAP_TOL:g}): the "
                f"weights are within N kkt_gap = {N * gap:.3g} of the optimal objective")
    return None


def compare_pointwise(elpd_i: Dict[str, np.ndarray], method: str = "stacking", b_samples: int = 1000, seed: int = 0, p=None, warning=None,
                      ic: str = "loo", device: Optional[int] = None) -> dict:
    """{model name: pointwise elpd (N,)} -> the columns of `az.compare`'s frame, ranked by elpd (best first): names, rank,
    elpd_<ic>, p_<ic>, elpd_diff, weight, se, dse, warning, scale = "log".  `p` and `warning`: {name: value} carried into the columns
    (NaN / False where absent).  Under "BB-pseudo-BMA" `se` is the bootstrap's se_bb, as in ArviZ; under "stacking" the result also
    has `kkt_gap` and `passes`, and a UserWarning is raised when the solver stopped at its cap of 64 passes with a larger gap
    than 1e-10.  A non-finite value in any row is refused."""
    if method not in METHODS:
        raise ValueError(f"compare: method must be one of {METHODS}, not {method!r}")
    if ic not in ("loo", "waic"):
        raise ValueError(f"compare: ic must be 'loo' or 'waic', not {ic!r}")
    names = list(elpd_i)
    K = len(names)
    if K < 2:
        raise ValueError(f"compare: at least 2 models, not {K}")
    if K > MAX_MODELS:
        raise ValueError(f"compare: at most {MAX_MODELS} models, not {K}")
    rows = [np.ascontiguousarray(elpd_i[n], dtype="float64").reshape(-1) for n in names]
    sizes = {n: r.size for n, r in zip(names, rows)}
    if len(set(sizes.values())) != 1:
        raise ValueError(f"compare: the models must have the same number of observations, not {sizes}")
    if method == "BB-pseudo-BMA" and not 1 <= int(b_samples) <= 65536:
        raise ValueError(f"compare: b_samples must lie in 1 .. 65536, not {b_samples}")
    N = rows[0].size
    extra = {}
    with Comparison(N, K, device) as c:
        for k, r in enumerate(rows):
            c.set(k, r)
        elpd, se, dse, best = c.moments()
        if method == "stacking":
            weight, _, gap, passes = c.stacking()
            extra = {"kkt_gap": gap, "passes": passes}
            text = cap_warning(gap, passes, N)
            if text:
                warnings.warn(text, UserWarning, stacklevel=2)
        elif method == "BB-pseudo-BMA":
            weight, se = c.bb(b_samples, seed)
        else:
            weight = pseudo_bma_weights(elpd)
    rank = sorted(range(K), key=lambda k: (-elpd[k], k))          # (stable: ties keep the caller's order, the best one first)
    p = p or {}
    warning = warning or {}
    out = {
        "names": [names[k] for k in rank],
        "rank": np.arange(K),
        f"elpd_{ic}": elpd[rank],
        f"p_{ic}": np.array([float(p.get(names[k], np.nan)) for k in rank]),
        "elpd_diff": elpd[best] - elpd[rank],
        "weight": weight[rank],
        "se": se[rank],
        "dse": dse[rank],
        "warning": [bool(warning.get(names[k], False)) for k in rank],
        "scale": "log",
        "method": method,
    }
    out.update(extra)
    return out


def compare(models: dict, ic: str = "loo", var_name=None, reff: float = 1.0, method: str = "stacking", b_samples: int = 1000, seed: int = 0,
            device: Optional[int] = None) -> dict:
    """{name: (model, draws)} -> `compare_pointwise` of the models' pointwise `loglik.loo` (ic = "loo") or `loglik.waic` ("waic"),
    computed one model after the other: only the N-vectors are alive together.  `var_name` names the observed variable in every
    model (one name for all of them); `reff` as in `loglik.loo`."""
    from pymc_amd import loglik

    if ic not in ("loo", "waic"):
        raise ValueError(f"compare: ic must be 'loo' or 'waic', not {ic!r}")
    if method not in METHODS:
        raise ValueError(f"compare: method must be one of {METHODS}, not {method!r}")
    rows, p, warn = {}, {}, {}
    for name, (model, draws) in models.items():
        if ic == "loo":
            r = loglik.loo(model, draws, var_name=var_name, pointwise=True, reff=reff, device=device)
            rows[name], p[name] = r["loo_i"], r["p_loo"]
        else:
            r = loglik.waic(model, draws, var_name=var_name, pointwise=True, device=device)
            rows[name], p[name] = r["waic_i"], r["p_waic"]
        warn[name] = r["warning"]
    sizes = {n: int(np.size(v)) for n, v in rows.items()}
    if len(set(sizes.values())) > 1:
        raise ValueError(f"compare: the models must have the same number of observations, not {sizes}")
    return compare_pointwise(rows, method=method, b_samples=b_samples, seed=seed, p=p, warning=warn, ic=ic, device=device)
