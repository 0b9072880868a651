"""`ValueGradFunction` stand-in backed by the HIP model kernels.

Replaces the compiled artefact of pymc/model/core.py:142-305: a callable
``f(q: float64[n]) -> (logp: float64 scalar, dlogp: float64[n])`` over the
unconstrained, raveled, concatenated value variables.  Exposes the attributes
the integrator reads (`_raveled_inputs`, `dtype`, `_extra_vars_shared`,
`_pytensor_function`; pymc/step_methods/hmc/integration.py:46-61,
pymc/step_methods/arraystep.py:205).
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.linalg

from pymc_amd import _lib
from pymc_amd.blocking import DictToArrayBijection, RaveledVars
from pymc_amd.model_spec import ModelSpec


def _pack(spec: ModelSpec, rows_group_aligned: bool = True):
    """ModelSpec -> nuts_model_spec (+ the numpy buffers that must outlive the call)."""
    keep = []
    data = spec.data if getattr(spec, "n_device_data", None) is None else spec.data[: spec.n_device_data]   # (the rest: host-only constants of Deterministics)
    nv, nf, nd = len(spec.vars), len(spec.factors), len(data)
    vars_c = (_lib.Var * max(nv, 1))()
    for i, v in enumerate(spec.vars):
        vars_c[i] = _lib.Var(v.offset, v.size, v.transform, 0, v.lower, v.upper)
    fac_c = (_lib.Factor * max(nf, 1))()
    n_instr = sum(len(getattr(f, "prog", ())) for f in spec.factors)
    ins_c = (_lib.Instr * max(n_instr, 1))()
    ioff = 0
    for i, f in enumerate(spec.factors):
        fc = _lib.Factor()
        fc.dist, fc.size, fc.nargs, fc.konst = f.dist, f.size, len(f.args), f.konst
        for k, t in enumerate(f.args):
            for nm in ("a", "b", "c"):
                o = getattr(t, nm)
                setattr(fc.arg[k], nm, _lib.Operand(o.kind, max(o.ref, 0), o.c))
        prog = getattr(f, "prog", ())
        fc.n_instr, fc.instr_off = len(prog), ioff
        for ins in prog:
            z = getattr(ins, "z", None) or ins.y
            ins_c[ioff] = _lib.Instr(ins.op, 0, ins.k, _lib.Operand(ins.x.kind, max(ins.x.ref, 0), ins.x.c), _lib.Operand(ins.y.kind, max(ins.y.ref, 0), ins.y.c),
                                     _lib.Operand(z.kind, max(z.ref, 0), z.c))
            ioff += 1
        fac_c[i] = fc
    refs = (_lib.DataRef * max(nd, 1))()
    off = 0
    for i, d in enumerate(data):
        refs[i] = _lib.DataRef(off, d.size)
        off += d.size
    pool = np.concatenate(data).astype("float64") if nd else np.zeros(1)
    keep += [vars_c, fac_c, refs, pool, ins_c]
    s = _lib.ModelSpecC()
    s.instrs, s.n_instrs = (ins_c if n_instr else None), n_instr
    s.n_vars, s.n_factors, s.n_data = nv, nf, nd
    s.vars, s.factors, s.data = vars_c, fac_c, refs
    s.data_pool, s.data_pool_len = _lib.dptr(pool), off
    if spec.logit_rows is not None:
        r = spec.logit_rows
        X = np.ascontiguousarray(r.X, dtype="float64")
        y = np.ascontiguousarray(r.y, dtype="int8")
        g = np.ascontiguousarray(r.group_idx, dtype="int32")
        keep += [X, y, g]
        s.rows_N, s.rows_D = X.shape
        s.rows_G = spec.vars[r.z].size // X.shape[1]
        s.rows_X = _lib.dptr(X)
        s.rows_y = y.ctypes.data_as(C.POINTER(C.c_int8))
        s.rows_gid = g.ctypes.data_as(C.POINTER(C.c_int32))
        s.rows_mu, s.rows_sigma, s.rows_z = r.mu, r.sigma, r.z
        s.rows_opts = 0 if rows_group_aligned else 1   # NUTS_ROWS_NO_GROUP_ALIGNED
    if spec.mvnormal is not None:
        mv = spec.mvnormal
        # Cholesky + triangular solves, as quaddist_chol does (pymc/distributions/multivariate.py:165-185);
        # the device consumes the precision matrix so one leapfrog is a single symmetric mat-vec.
        L = scipy.linalg.cholesky(mv.cov, lower=True)
        prec = np.ascontiguousarray(scipy.linalg.cho_solve((L, True), np.eye(len(mv.mu))))
        prec = 0.5 * (prec + prec.T)
        mu = np.ascontiguousarray(mv.mu, dtype="float64")
        keep += [prec, mu]
        s.mvn_var, s.mvn_k = mv.var, len(mu)
        s.mvn_mu, s.mvn_prec = _lib.dptr(mu), _lib.dptr(prec)
        s.mvn_logdet = float(np.log(np.diag(L)).sum())
        if getattr(mv, "solver", "precision") == "cholesky":
            winv = np.ascontiguousarray(np.tril(scipy.linalg.solve_triangular(L, np.eye(len(mu)), lower=True)))
            keep.append(winv)
            s.mvn_winv = _lib.dptr(winv)
    mx = getattr(spec, "mixture_rows", None)
    if mx is not None:
        y = np.ascontiguousarray(mx.y, dtype="float64")
        keep.append(y)
        s.mix_N, s.mix_K, s.mix_mu = y.size, mx.K, mx.mu
        s.mix_y = _lib.dptr(y)
        s.mix_sigma = -1 if mx.sigma is None else mx.sigma
        s.mix_w_logits = -1 if mx.w_logits is None else mx.w_logits
        s.mix_assign = -1 if mx.assign is None else mx.assign
        if mx.sigma is None:
            sc = np.ascontiguousarray(mx.sigma_const, dtype="float64")
            keep.append(sc)
            s.mix_sigma_const = _lib.dptr(sc)
        if mx.w_logits is None:
            wc = np.ascontiguousarray(mx.w_const, dtype="float64")
            keep.append(wc)
            s.mix_w_const = _lib.dptr(wc)
        elif getattr(mx, "w_alpha", None) is not None:
            wa = np.ascontiguousarray(mx.w_alpha, dtype="float64")
            keep.append(wa)
            s.mix_w_simplex = 1
            s.mix_w_alpha = _lib.dptr(wa)
    gl = getattr(spec, "glm_rows", None)
    if gl is not None:
        X = np.ascontiguousarray(gl.X, dtype="float64")
        y = np.ascontiguousarray(gl.y, dtype="float64")
        keep += [X, y]
        s.glm_N, s.glm_P = X.shape
        s.glm_family = gl.family
        s.glm_beta = -1 if gl.beta is None else gl.beta
        s.glm_beta_derived = -1 if getattr(gl, "beta_derived", None) is None else gl.beta_derived
        s.glm_intercept = -1 if gl.intercept is None else gl.intercept
        s.glm_sigma = -1 if gl.sigma is None else gl.sigma
        s.glm_sigma_const = float(gl.sigma_const)
        s.glm_X, s.glm_y = _lib.dptr(X), _lib.dptr(y)
    lins = getattr(spec, "lins", None) or []
    if lins:
        lins_c = (_lib.Lin * len(lins))()
        for i, L in enumerate(lins):
            X = np.ascontiguousarray(L.X, dtype="float64")
            keep.append(X)
            lins_c[i].N, lins_c[i].P = X.shape
            lins_c[i].K = len(L.cols)
            lins_c[i].X = _lib.dptr(X)
            for k, (var, off_, stride) in enumerate(L.cols[:16]):
                lins_c[i].var[k], lins_c[i].off[k], lins_c[i].stride[k] = var, off_, stride
        keep.append(lins_c)
        s.n_lins, s.lins = len(lins), lins_c
    return s, keep


class DeviceValueGradFunction:
    """Device-resident logp/dlogp function of a :class:`ModelSpec`."""

    def __init__(self, spec: ModelSpec, device: int | None = None, rows_group_aligned: bool = True):
        lib = _lib.load()
        if device is not None:
            _lib.check(lib.nuts_set_device(int(device)), "nuts_set_device")
        self.spec = spec
        self.device = device
        self.dtype = "float64"
        self._raveled_inputs = True
        self._extra_vars_shared = {}
        self._extra_are_set = False
        self.trust_input = True
        self.rows_group_aligned_allowed = rows_group_aligned
        cspec, keep = _pack(spec, rows_group_aligned)
        _lib.sync_options_from_env()     # (tests / tools only: see _lib.py)
        self._handle = lib.nuts_model_create(C.byref(cspec))
        del keep
        if not self._handle:
            raise _lib.EngineError(f"nuts_model_create failed: {_lib.last_error()}")
        self.n = lib.nuts_model_ndim(self._handle)
        self._grad = np.empty(self.n)
        self._lp = np.empty(1)

    def model_scalar(self, name: str) -> float:
        out = C.c_double()
        _lib.check(_lib.load().nuts_model_get_scalar(self._handle, name.encode(), C.byref(out)), name)
        return out.value

    def bind_thread(self):
        """HIP's current device is per host thread: a worker thread that drives this model selects its device first."""
        if self.device is not None:
            _lib.check(_lib.load().nuts_set_device(int(self.device)), "nuts_set_device")

    # the integrator calls `_pytensor_function(q)` directly (integration.py:46-52)
    def _pytensor_function(self, q):
        q = np.ascontiguousarray(q, dtype="float64")
        grad = np.empty(self.n)
        lp = np.empty(1)
        rc = _lib.load().nuts_model_logp_grad(self._handle, _lib.dptr(q), _lib.dptr(lp), _lib.dptr(grad))
        _lib.check(rc, "nuts_model_logp_grad")
        return lp[0], grad

    def __call__(self, grad_vars, *, extra_vars=None):
        """`ValueGradFunction.__call__` (pymc/model/core.py:286-300)."""
        if extra_vars is not None:
            self.set_extra_values(extra_vars)
        elif self.spec.extra and not self._extra_are_set:
            raise ValueError("Extra values are not set.")
        if isinstance(grad_vars, RaveledVars):
            q = grad_vars.data
        elif isinstance(grad_vars, dict):
            q = DictToArrayBijection.map({v.value_name: grad_vars[v.value_name] for v in self.spec.vars}).data
        else:
            q = np.asarray(grad_vars[0] if isinstance(grad_vars, (list, tuple)) else grad_vars)
        return self._pytensor_function(q)

    def set_extra_values(self, extra_vars):
        """core.py:275-278: the non-gradient inputs are data vectors of the spec, rewritten on the device
        (`nuts_model_set_data`; values that did not change are not sent again)."""
        lib = _lib.load()
        ids, vals = [], []
        for name, idx in self.spec.extra.items():
            v = np.ascontiguousarray(np.asarray(extra_vars[name], dtype="float64").ravel())
            old = self._extra_vars_shared.get(name)
            if old is not None and old.shape == v.shape and np.array_equal(old, v):
                continue
            ids.append(idx)
            vals.append(v)
            self._extra_vars_shared[name] = v.copy()
        if ids:     # ONE call, stream-ordered (no host synchronisation per vector)
            ids_a = np.asarray(ids, dtype="int32")
            lens = np.asarray([v.size for v in vals], dtype="int64")
            flat = np.concatenate(vals) if len(vals) > 1 else vals[0]
            _lib.check(lib.nuts_model_set_data_many(self._handle, len(ids), ids_a.ctypes.data, _lib.dptr(flat), lens.ctypes.data), "nuts_model_set_data_many")
        self._extra_are_set = True

    def get_extra_values(self):  # core.py:280-284
        if self.spec.extra and not self._extra_are_set:
            raise ValueError("Extra values are not set.")
        return {name: self._extra_vars_shared[name].copy() for name in self.spec.extra}

    def _ll_node(self, name, node):
        if node is not None:
            return int(node[0]), int(node[1])
        from pymc_amd.model_spec import observed_nodes

        for nm, kind, index, _ in observed_nodes(self.spec):
            if nm == name:
                return kind, index
        raise KeyError(f"{name!r} is not an observed variable of the model")

    def log_likelihood(self, name: str, q, node=None) -> np.ndarray:
        """Element-wise log-likelihood of observed variable `name` at the raveled unconstrained draws q [S, n] -> [S, size]
        (`nuts_model_loglik`; logit rows in the spec's group-sorted order).  `node`: (kind, index) when the caller knows it."""
        lib = _lib.load()
        kind, index = self._ll_node(name, node)
        q = np.ascontiguousarray(np.asarray(q, dtype="float64").reshape(-1, self.n))
        size = C.c_int64()
        _lib.check(lib.nuts_model_loglik_size(self._handle, kind, index, C.byref(size)), "nuts_model_loglik_size")
        out = np.empty((q.shape[0], size.value))
        _lib.check(lib.nuts_model_loglik(self._handle, kind, index, _lib.dptr(q), q.shape[0], _lib.dptr(out)), "nuts_model_loglik")
        return out

    def logdens_sum(self, q, node) -> np.ndarray:
        """The total of node (kind, index)'s pointwise values at each raveled unconstrained draw q [S, n] -> [S], reduced on the device
        (`nuts_model_logdens_sum`): what `log_likelihood(...).sum(axis=1)` would give, without the [S, size] matrix."""
        lib = _lib.load()
        kind, index = int(node[0]), int(node[1])
        q = np.ascontiguousarray(np.asarray(q, dtype="float64").reshape(-1, self.n))
        out = np.empty(q.shape[0])
        _lib.check(lib.nuts_model_logdens_sum(self._handle, kind, index, _lib.dptr(q), q.shape[0], _lib.dptr(out)), "nuts_model_logdens_sum")
        return out

    def waic_accumulator(self, name: str, node=None) -> "WaicAccumulator":
        """Device-resident per-observation WAIC accumulators of observed variable `name` (`nuts_waic_*`)."""
        kind, index = self._ll_node(name, node)
        return WaicAccumulator(self, kind, index)

    def psis_accumulator(self, name: str, n_draws: int, reff: float = 1.0, node=None) -> "PsisAccumulator":
        """Device-resident per-observation PSIS-LOO state of observed variable `name` for a trace of `n_draws` pooled draws
        (`nuts_psis_*`)."""
        kind, index = self._ll_node(name, node)
        return PsisAccumulator(self, kind, index, n_draws, reff)

    def posterior_predictive(self, name: str, q, seed: int = 0, draw0: int = 0, node=None) -> np.ndarray:
        """One replicate of observed variable `name` per raveled unconstrained draw q [S, n] -> [S, size] (`nuts_model_predictive`;
        logit rows in the spec's group-sorted order).  Draw s of the call is draw `draw0 + s` of the generator's stream under `seed`."""
        lib = _lib.load()
        kind, index = self._ll_node(name, node)
        q = np.ascontiguousarray(np.asarray(q, dtype="float64").reshape(-1, self.n))
        size = C.c_int64()
        _lib.check(lib.nuts_model_loglik_size(self._handle, kind, index, C.byref(size)), "nuts_model_loglik_size")
        out = np.empty((q.shape[0], size.value))
        rc = lib.nuts_model_predictive(self._handle, kind, index, _lib.dptr(q), q.shape[0], int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw0), _lib.dptr(out))
        _lib.check(rc, "nuts_model_predictive")
        return out

    def prior(self, S: int, seed: int = 0, draw0: int = 0):
        """S raveled UNCONSTRAINED positions drawn from the priors of the free variables, in ancestral order (`nuts_model_prior`)
        -> (q [S, n], number of non-finite entries of q).  Draw s of the call is draw `draw0 + s` of the generator's stream under
        `seed`; the result does not depend on how S is split over calls."""
        out = np.empty((int(S), self.n))
        bad = C.c_int64()
        rc = _lib.load().nuts_model_prior(self._handle, int(S), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw0), _lib.dptr(out), C.byref(bad))
        _lib.check(rc, "nuts_model_prior")
        return out, int(bad.value)

    def ppc_accumulator(self, name: str, seed: int = 0, node=None) -> "PpcAccumulator":
        """Device-resident streaming predictive checks of observed variable `name` (`nuts_ppc_*`)."""
        kind, index = self._ll_node(name, node)
        return PpcAccumulator(self, kind, index, seed)

    def predict_moments(self, name: str, q, node=None, var: bool = True):
        """Conditional mean and variance of observed variable `name` per raveled unconstrained draw q [S, n] -> (mean [S, size],
        var [S, size] or None) (`nuts_model_predict_moments`; logit rows in the spec's group-sorted order).  The function is that of
        a spec carrying the rows to predict at (`model_spec.with_data`)."""
        lib = _lib.load()
        kind, index = self._ll_node(name, node)
        q = np.ascontiguousarray(np.asarray(q, dtype="float64").reshape(-1, self.n))
        size = C.c_int64()
        _lib.check(lib.nuts_model_loglik_size(self._handle, kind, index, C.byref(size)), "nuts_model_loglik_size")
        mean = np.empty((q.shape[0], size.value))
        v = np.empty((q.shape[0], size.value)) if var else None
        rc = lib.nuts_model_predict_moments(self._handle, kind, index, _lib.dptr(q), q.shape[0], _lib.dptr(mean), _lib.dptr(v) if var else None)
        _lib.check(rc, "nuts_model_predict_moments")
        return mean, v

    def pred_accumulator(self, name: str, with_y: bool = True, node=None) -> "PredAccumulator":
        """Device-resident streaming predictions of observed variable `name` (`nuts_pred_*`); `with_y`: the node's observed
        values are held-out values, whose log predictive density is folded too."""
        kind, index = self._ll_node(name, node)
        return PredAccumulator(self, kind, index, with_y)

    def loo_pit_accumulator(self, psis_accumulator: "PsisAccumulator", seed: int = 0) -> "LooPitAccumulator":
        """Device-resident LOO predictive checks of the observed variable of `psis_accumulator`, which must hold all of its draws:
        the second pass over them (`nuts_loo_pit_*`)."""
        if psis_accumulator._func is not self:
            raise ValueError("the PSIS accumulator belongs to another function")
        return LooPitAccumulator(psis_accumulator, seed)

    def time_kernels(self, q, reps=20):
        ms_tot, ms_dom = C.c_double(), C.c_double()
        q = np.ascontiguousarray(q, dtype="float64")
        rc = _lib.load().nuts_model_time_logp_grad(self._handle, _lib.dptr(q), reps, C.byref(ms_tot), C.byref(ms_dom))
        _lib.check(rc, "nuts_model_time_logp_grad")
        return ms_tot.value, ms_dom.value

    @property
    def algorithmic_bytes(self) -> int:
        return int(_lib.load().nuts_model_algorithmic_bytes(self._handle))

    def close(self):
        if getattr(self, "_handle", None):
            _lib.load().nuts_model_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WaicAccumulator:
    """`nuts_waic`: (m, r, mean, M2) per observation, updated by any number of `update(q [S, n])` calls in any split."""

    def __init__(self, func: DeviceValueGradFunction, kind: int, index: int):
        lib = _lib.load()
        self._func = func      # (the handle must not outlive its model)
        size = C.c_int64()
        _lib.check(lib.nuts_model_loglik_size(func._handle, kind, index, C.byref(size)), "nuts_model_loglik_size")
        self.size = size.value
        self._handle = lib.nuts_waic_create(func._handle, kind, index)
        if not self._handle:
            raise ValueError(f"nuts_waic_create: {_lib.last_error()}")

    def update(self, q) -> None:
        q = np.ascontiguousarray(np.asarray(q, dtype="float64").reshape(-1, self._func.n))
        _lib.check(_lib.load().nuts_waic_update(self._handle, _lib.dptr(q), q.shape[0]), "nuts_waic_update")

    def read(self):
        """(lppd_i, p_waic_i, draws so far)"""
        lppd, p = np.empty(self.size), np.empty(self.size)
        n = C.c_int64()
        _lib.check(_lib.load().nuts_waic_read(self._handle, _lib.dptr(lppd), _lib.dptr(p), C.byref(n)), "nuts_waic_read")
        return lppd, p, n.value

    def raw(self):
        """(the accumulators [4, size]: m, r, mean, M2; draws so far)"""
        acc = np.empty((4, self.size))
        n = C.c_int64()
        lib = _lib.load()
        _lib.check(lib.nuts_waic_read_raw(self._handle, _lib.dptr(acc)), "nuts_waic_read_raw")
        _lib.check(lib.nuts_waic_read(self._handle, None, None, C.byref(n)), "nuts_waic_read")
        return acc, n.value

    def close(self):
        if getattr(self, "_handle", None):
            _lib.load().nuts_waic_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PsisAccumulator:
    """`nuts_psis`: per observation the tail of the importance ratios (the M + 1 smallest log-likelihood values) and the running
    log-sum of the rest, updated by `update(q [S, n])` calls in any split until `n_draws` are in; `read()` then fits and smooths."""

    def __init__(self, func: DeviceValueGradFunction, kind: int, index: int, n_draws: int, reff: float = 1.0):
        lib = _lib.load()
        self._func = func      # (the handle must not outlive its model)
        size = C.c_int64()
        _lib.check(lib.nuts_model_loglik_size(func._handle, kind, index, C.byref(size)), "nuts_model_loglik_size")
        self.size = size.value
        self.n_draws = int(n_draws)
        self._handle = lib.nuts_psis_create(func._handle, kind, index, self.n_draws, float(reff))
        if not self._handle:
            raise ValueError(f"nuts_psis_create: {_lib.last_error()}")

    def update(self, q) -> None:
        q = np.ascontiguousarray(np.asarray(q, dtype="float64").reshape(-1, self._func.n))
        _lib.check(_lib.load().nuts_psis_update(self._handle, _lib.dptr(q), q.shape[0]), "nuts_psis_update")

    def read(self):
        """(elpd_loo_i, khat_i, lppd_i, draws): only once all `n_draws` are in"""
        elpd, khat, lppd = np.empty(self.size), np.empty(self.size), np.empty(self.size)
        n = C.c_int64()
        _lib.check(_lib.load().nuts_psis_read(self._handle, _lib.dptr(elpd), _lib.dptr(khat), _lib.dptr(lppd), C.byref(n)), "nuts_psis_read")
        return elpd, khat, lppd, n.value

    def raw(self):
        """(keep [K1, size] ascending per column, +inf where empty; acc [4, size]: m, r of ll, m_rest, r_rest of -ll; draws so far)"""
        lib = _lib.load()
        k1, n = C.c_int64(), C.c_int64()
        _lib.check(lib.nuts_psis_read_raw(self._handle, None, None, C.byref(k1)), "nuts_psis_read_raw")
        keep, acc = np.empty((k1.value, self.size)), np.empty((4, self.size))
        _lib.check(lib.nuts_psis_read_raw(self._handle, _lib.dptr(keep), _lib.dptr(acc), C.byref(k1)), "nuts_psis_read_raw")
        _lib.check(lib.nuts_psis_read(self._handle, None, None, None, C.byref(n)), "nuts_psis_read")
        return keep, acc, n.value

    def close(self):
        if getattr(self, "_handle", None):
            _lib.load().nuts_psis_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PpcAccumulator:
    """`nuts_ppc`: per observation (mean, M2) of the replicates and the counts below / at the observed value, per draw (sum, sum of
    squares, min, max) over the observations, updated by any number of `update(q [S, n])` calls in any split; the draws are
    numbered on from the handle's count."""

    def __init__(self, func: DeviceValueGradFunction, kind: int, index: int, seed: int = 0):
        lib = _lib.load()
        self._func = func      # (the handle must not outlive its model)
        size = C.c_int64()
        _lib.check(lib.nuts_model_loglik_size(func._handle, kind, index, C.byref(size)), "nuts_model_loglik_size")
        self.size = size.value
        self._handle = lib.nuts_ppc_create(func._handle, kind, index, int(seed) & 0xFFFFFFFFFFFFFFFF)
        if not self._handle:
            raise ValueError(f"nuts_ppc_create: {_lib.last_error()}")

    def update(self, q) -> None:
        q = np.ascontiguousarray(np.asarray(q, dtype="float64").reshape(-1, self._func.n))
        _lib.check(_lib.load().nuts_ppc_update(self._handle, _lib.dptr(q), q.shape[0]), "nuts_ppc_update")

    def read(self):
        """(mean_i, var_i = M2 / S, #{y_rep < y_i}, #{y_rep == y_i}, draws so far)"""
        mean, var, n_lt, n_eq = (np.empty(self.size) for _ in range(4))
        n = C.c_int64()
        rc = _lib.load().nuts_ppc_read(self._handle, _lib.dptr(mean), _lib.dptr(var), _lib.dptr(n_lt), _lib.dptr(n_eq), C.byref(n))
        _lib.check(rc, "nuts_ppc_read")
        return mean, var, n_lt, n_eq, n.value

    def stats(self):
        """(T [draws, 4]: sum, sum of squares, min, max of each draw's replicate; T_obs [4]: the same of the observed data)"""
        lib = _lib.load()
        n = C.c_int64()
        _lib.check(lib.nuts_ppc_read(self._handle, None, None, None, None, C.byref(n)), "nuts_ppc_read")
        T, T_obs = np.empty((n.value, 4)), np.empty(4)
        _lib.check(lib.nuts_ppc_read_stats(self._handle, _lib.dptr(T), _lib.dptr(T_obs)), "nuts_ppc_read_stats")
        return T, T_obs

    def close(self):
        if getattr(self, "_handle", None):
            _lib.load().nuts_ppc_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PredAccumulator:
    """`nuts_pred`: per observation Welford's (mean, M2) of the conditional mean, the running mean of the conditional variance and
    the running log-sum-exp of the held-out log-density, updated by any number of `update(q [S, n])` calls in any split."""

    def __init__(self, func: DeviceValueGradFunction, kind: int, index: int, with_y: bool = True):
        lib = _lib.load()
        self._func = func      # (the handle must not outlive its model)
        size = C.c_int64()
        _lib.check(lib.nuts_model_loglik_size(func._handle, kind, index, C.byref(size)), "nuts_model_loglik_size")
        self.size = size.value
        self.with_y = bool(with_y)
        self._handle = lib.nuts_pred_create(func._handle, kind, index, int(self.with_y))
        if not self._handle:
            raise ValueError(f"nuts_pred_create: {_lib.last_error()}")

    def update(self, q) -> None:
        q = np.ascontiguousarray(np.asarray(q, dtype="float64").reshape(-1, self._func.n))
        _lib.check(_lib.load().nuts_pred_update(self._handle, _lib.dptr(q), q.shape[0]), "nuts_pred_update")

    def read(self):
        """(mean_i, var_between_i = M2 / S, var_within_i, lpd_i or None, draws so far)"""
        mean, vb, vw = (np.empty(self.size) for _ in range(3))
        lpd = np.empty(self.size) if self.with_y else None
        n = C.c_int64()
        rc = _lib.load().nuts_pred_read(self._handle, _lib.dptr(mean), _lib.dptr(vb), _lib.dptr(vw), _lib.dptr(lpd) if self.with_y else None, C.byref(n))
        _lib.check(rc, "nuts_pred_read")
        return mean, vb, vw, lpd, n.value

    def close(self):
        if getattr(self, "_handle", None):
            _lib.load().nuts_pred_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LooPitAccumulator:
    """`nuts_loo_pit`: the second pass over the draws of a finished `PsisAccumulator` (which it borrows and keeps alive).  Per
    observation the sums of the Pareto-smoothed weights w, of w^2, of w over the replicates below / at the observed value, and the
    weighted mean and variance of the replicates; `update(q [S, n], draw0)` in any split, the replicate of a draw addressed by its
    global number `draw0` + position."""

    def __init__(self, psis: PsisAccumulator, seed: int = 0):
        lib = _lib.load()
        self._psis = psis      # (the handle borrows its sorted column and must not outlive it)
        self._func = psis._func
        self.size = psis.size
        if not getattr(psis, "_handle", None):
            raise ValueError("nuts_loo_pit_create: the PSIS accumulator is closed")
        self._handle = lib.nuts_loo_pit_create(psis._handle, int(seed) & 0xFFFFFFFFFFFFFFFF)
        if not self._handle:
            raise ValueError(f"nuts_loo_pit_create: {_lib.last_error()}")

    def _live(self):
        if not getattr(self._psis, "_handle", None):
            raise ValueError("the PSIS accumulator this pass reads from was closed")

    def update(self, q, draw0: int = 0) -> None:
        self._live()
        q = np.ascontiguousarray(np.asarray(q, dtype="float64").reshape(-1, self._func.n))
        _lib.check(_lib.load().nuts_loo_pit_update(self._handle, _lib.dptr(q), q.shape[0], int(draw0)), "nuts_loo_pit_update")

    def read(self):
        """(p_lt, p_eq, mean, var, sum_w, sum_w2, draws so far); NaN in every column where the fit is degenerate or poisoned"""
        self._live()
        p_lt, p_eq, mean, var, sum_w, sum_w2 = (np.empty(self.size) for _ in range(6))
        n = C.c_int64()
        rc = _lib.load().nuts_loo_pit_read(self._handle, _lib.dptr(p_lt), _lib.dptr(p_eq), _lib.dptr(mean), _lib.dptr(var), _lib.dptr(sum_w),
                                           _lib.dptr(sum_w2), C.byref(n))
        _lib.check(rc, "nuts_loo_pit_read")
        return p_lt, p_eq, mean, var, sum_w, sum_w2, n.value

    def close(self):
        if getattr(self, "_handle", None):
            _lib.load().nuts_loo_pit_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
