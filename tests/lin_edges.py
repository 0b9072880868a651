"""What the linear-predictor edge tests share (tests/test_lin_edges.py, tests/test_gpu_lin_edges.py); needs no device.

Dense node 5 (pymc_amd/csrc/lin_kernel.h: `k_lin_fwd` / `k_lin_fwd1`, the adjoint sweep, `k_lin_bwd` / `k_lin_bwd1`, `k_lin_fin`) is
LINEAR in the coefficients.  One family of models serves every shape:

    likelihood          Potential("y",  sum_k -0.5 (y_k - eta_k)^2)          eta_k = X coef_k
    further readers     Potential("r1", sum_k 0.25 r eta_k), r = 1, 2, 3      (a column read by 1 + r factors: `lin_adj`)
    prior               Normal(0, 1) on every variable                        (HalfNormal(1) under the log transform where it says so)

  * `exact_model`: X in [-4, 4] and y in [-8, 8] integers, positions multiples of 1/8.  Every product and every partial sum is then
    a small dyadic number: the gradient does not depend on summation order, chunking or `KT`, and the device must return EXACT
    ARITHMETIC bit for bit.  A dropped, duplicated or shifted row changes an integer.
  * `real_model`: the same structure over `rng.normal` data and positions, with a log-transformed coefficient matrix and the
    non-centred `mu + exp(log_tau) z` form.  The reference treats the doubles as exact (integers over a power of two; `exp` by
    mpmath at 400 bits) and the device is held to a bound whose constant is COUNTED from the kernels (`rounding_count`).

`evaluate_exact` is the one reference of both; `Dy` is its arithmetic (arrays of integers times a power of two, which REFUSES to
round).  tests/test_lin_edges.py holds it to plain `fractions.Fraction` at small sizes.
"""
import functools
import math
import os
import sys
from dataclasses import dataclass, field
from fractions import Fraction
from typing import List, Optional, Tuple

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# ---- the kernels' shapes, restated (pymc_amd/csrc/lin_kernel.h, model_dev.h, engine.hip `launch_lin_forward`) ----------------------
FWD_THREADS = 256        # rows per workgroup of `k_lin_fwd`
FWD_MAX_GRID = 4096      # its grid is capped here: from N = 4096 * 256 + 1 on a thread takes a second row
LIN_CHUNK = 2048         # rows per workgroup of `k_lin_bwd`
LIN_MAXUSE = 4           # factors that may read one column
LIN_MAXP = 512
ONE_ROW_TRIP = 8 * 1024  # elements `k_lin_fwd1` / `k_lin_bwd1` walk per trip of their loops
U = 2.0 ** -53
MP_PREC = 400


def kt_of(K):
    """The instantiation of `k_lin_fwd<KT>` / `k_lin_bwd<KT>` that serves K columns."""
    return 1 if K == 1 else 2 if K == 2 else 4 if K <= 4 else 8 if K <= 8 else 16


def where(i):
    """Row i of a predictor, in the kernels' terms (for a failure message)."""
    grid = FWD_MAX_GRID * FWD_THREADS
    return (f"row {i}: forward workgroup {(i % grid) // FWD_THREADS}, thread {i % FWD_THREADS}, trip {i // grid}; "
            f"backward chunk {i // LIN_CHUNK}, thread {(i % LIN_CHUNK) % 256}, step {(i % LIN_CHUNK) // 256}")


# ---- arithmetic that refuses to round -----------------------------------------------------------------------------------------------
def _pow2(e):
    return Fraction(1 << e, 1) if e >= 0 else Fraction(1, 1 << -e)


class Dy:
    """An array of INTEGERS `m` times 2^e.  The integers are float64 (the exact family: every operation asserts that its result and
    its partial sums stay below 2^53, so that numpy's float64 arithmetic is exact whatever order it sums in) or Python integers in an
    object array (the real-valued family: no limit)."""

    def __init__(self, m, e):
        self.m, self.e = np.asarray(m), int(e)

    @property
    def big(self):
        return self.m.dtype == object

    @staticmethod
    def of(a, big=False):
        """The doubles `a`, taken as exact."""
        a = np.asarray(a, dtype="float64")
        assert np.all(np.isfinite(a))
        mant, ex = np.frexp(a)
        M, ex = np.ldexp(mant, 53).astype(np.int64), ex.astype(np.int64) - 53      # a == M 2^ex, exactly
        nz = M != 0
        low = np.where(nz, M & -M, 1)                                              # the lowest set bit of each mantissa
        e = int((ex + np.log2(low.astype("float64")).astype(np.int64))[nz].min()) if np.any(nz) else 0
        if not big:
            return Dy(np.ldexp(a, -e), e)._ok()
        ints = [(m_ << (x_ - e) if x_ >= e else m_ >> (e - x_)) if m_ else 0 for m_, x_ in zip(M.ravel().tolist(), ex.ravel().tolist())]   # (only zero bits leave)
        out = np.empty(len(ints), dtype=object)
        out[:] = ints
        return Dy(out.reshape(a.shape), e)

    @staticmethod
    def of_mpf(vals, shape):
        """mpmath numbers (binary: man * 2^exp), taken as exact."""
        parts = [(int(v.man) * (-1 if v._mpf_[0] else 1), int(v.exp)) if v != 0 else (0, 0) for v in vals]
        e = min([x for m_, x in parts if m_] or [0])
        out = np.empty(len(parts), dtype=object)
        out[:] = [m_ << (x - e) if m_ else 0 for m_, x in parts]
        return Dy(out.reshape(shape), e)

    def _ok(self, mag=None):
        if not self.big:
            mag = np.abs(self.m) if mag is None else mag
            assert mag.size == 0 or float(np.max(mag)) < 2.0 ** 53, "the exact family left the range in which float64 is exact"
        return self

    def _at(self, e):
        k = self.e - e
        assert k >= 0
        if k == 0:
            return self.m
        return self.m * (1 << k) if self.big else Dy(self.m * 2.0 ** k, e)._ok().m

    def _pair(self, o):
        o = o if isinstance(o, Dy) else Dy.of(o, self.big)
        if self.big != o.big:
            raise TypeError("Dy: float64 integers and Python integers do not mix")
        e = min(self.e, o.e)
        return self._at(e), o._at(e), e, o

    def __add__(self, o):
        a, b, e, _ = self._pair(o)
        return Dy(a + b, e)._ok()

    def __sub__(self, o):
        a, b, e, _ = self._pair(o)
        return Dy(a - b, e)._ok()

    def __neg__(self):
        return Dy(-self.m, self.e)

    def __mul__(self, o):
        o = o if isinstance(o, Dy) else Dy.of(o, self.big)
        return Dy(self.m * o.m, self.e + o.e)._ok()

    def __matmul__(self, o):
        out = Dy(self.m @ o.m, self.e + o.e)
        return out if self.big else out._ok(np.abs(self.m) @ np.abs(o.m))

    def sum(self, axis=None):
        out = Dy(self.m.sum(axis=axis), self.e)
        return out if self.big else out._ok(np.abs(self.m).sum(axis=axis))

    @property
    def T(self):
        return Dy(self.m.T, self.e)

    def __getitem__(self, ix):
        return Dy(self.m[ix], self.e)

    def reshape(self, *shape):
        return Dy(self.m.reshape(*shape), self.e)

    def fractions(self):
        s = _pow2(self.e)
        return [Fraction(int(v)) * s for v in np.asarray(self.m).ravel().tolist()]

    def floats(self):
        """The values as float64: EXACT for the float64 kind, correctly rounded for the other."""
        if not self.big:
            return np.ldexp(self.m, self.e)
        return np.array([float(f) for f in self.fractions()]).reshape(self.m.shape)


# ---- the models ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Reader:
    """A factor that reads columns `cols` of predictor `pred`: kind "sq": sum_k -0.5 (y[:, k] - eta_k)^2 over M elements; kind "lin":
    sum_k w eta_k over M elements.  M is the predictor's N, or any size when the predictor has ONE row (it broadcasts)."""
    name: str
    pred: int
    cols: Tuple[int, ...]
    kind: str
    M: int
    y: Optional[np.ndarray] = None
    w: float = 0.0


@dataclass
class LinModel:
    spec: object
    coef: str                      # "var" | "log" | "derived" | "derived_log"
    P: int
    K: int
    Xs: List[np.ndarray]           # predictor l is Xs[l] @ B (all K columns)
    readers: List[Reader] = field(default_factory=list)
    exact: bool = True
    label: str = ""

    @property
    def n(self):
        return self.spec.n

    def factor_index(self, name="y"):
        return next(i for i, f in enumerate(self.spec.factors) if f.name == name)


def _build(coef, P, K, Xs, readers, exact, label):
    """The spec of the family through the builder (`m.dot`, OP_LIN operands), as tests/test_lin_node.py writes its models."""
    from pymc_amd.model_spec import ModelBuilder

    m = ModelBuilder()
    if coef in ("var", "log"):
        shape = (P,) if K == 1 else (P, K)
        B = m.Normal("B", 0.0, 1.0, shape=shape) if coef == "var" else m.HalfNormal("B", 1.0, shape=shape)
    else:
        assert K == 1
        mu = m.Normal("mu", 0.0, 1.0)
        tau = m.Normal("tau", 0.0, 1.0) if coef == "derived" else m.HalfNormal("tau", 1.0)
        z = m.Normal("z", 0.0, 1.0, shape=(P,))
        B = mu + tau * z
    etas = []
    for X in Xs:
        e = m.dot(X, B)
        etas.append(e if isinstance(e, list) else [e])
    for r in readers:
        N = Xs[r.pred].shape[0]
        assert r.M == N or N == 1
        total = None
        for j, k in enumerate(r.cols):
            eta = etas[r.pred][k]
            if r.kind == "sq":
                term = (m.as_expr(np.ascontiguousarray(r.y[:, j])) - eta) ** 2 * -0.5
            else:
                term = eta * r.w if N > 1 else m.as_expr(np.full(r.M, r.w)) * eta
            total = term if total is None else total + term
        m.Potential(r.name, total)
    return LinModel(m.build(), coef, P, K, [np.asarray(X, dtype="float64") for X in Xs], list(readers), exact, label)


def _draw(rng, exact, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype("float64") if exact else rng.normal(size=shape) * (hi / 2.0)


def _family(exact, N, P, K=1, readers=1, unread=(), coef="var", reader_cols=None, N2=None, M=None, M2=None, seed=0):
    """N > 1: K columns over X [N, P]; `readers` factors read every column not in `unread` (the further ones only `reader_cols`
    where given); `N2`: a SECOND predictor X2 [N2, P] over the same coefficients with a likelihood of its own (`LinTarget.n_src` = 2).
    N == 1: a one-row predictor that broadcasts into a likelihood of M elements; `M2`: a second reader, of M2 elements."""
    rng = np.random.default_rng([seed, N, P, K, readers, 1 if exact else 0])
    Xs = [_draw(rng, exact, (N, P), -4, 4)]
    read = tuple(k for k in range(K) if k not in unread)
    M = N if N > 1 else (M or 7)
    rs = [Reader("y", 0, read, "sq", M, y=_draw(rng, exact, (M, len(read)), -8, 8))]
    if N > 1:
        for r in range(1, readers):
            rs.append(Reader(f"r{r}", 0, tuple(reader_cols) if reader_cols is not None else read, "lin", N, w=0.25 * r))
        if N2:
            Xs.append(_draw(rng, exact, (N2, P), -4, 4))
            rs.append(Reader("y2", 1, read, "sq", N2, y=_draw(rng, exact, (N2, len(read)), -8, 8)))
    elif M2:
        rs.append(Reader("r1", 0, read, "lin", M2, w=0.25))
    label = f"N{N}-P{P}-K{K}-readers{readers}-{coef}" + (f"-unread{list(unread)}" if unread else "") + (f"-M{M}" if N == 1 else "")
    return _build(coef, P, K, Xs, rs, exact, label)


def exact_model(N, P, K=1, readers=1, unread=(), coef="var", **kw):
    """The integer family: see the module's docstring.  `coef` = "derived": coefficients `mu + tau z`, mu and tau scalar Normal
    variables (tau an UNTRANSFORMED multiplier), z a vector; at positions that are multiples of 1/8 the products are multiples of 1/64."""
    assert coef in ("var", "derived")
    return _family(True, N, P, K, readers, unread, coef, **kw)


def real_model(N, P, K=1, readers=1, coef="var", **kw):
    """The same structure over `rng.normal` data.  `coef` = "log": a HalfNormal coefficient matrix under the log transform;
    "derived_log": `mu + exp(log_tau) z`, the non-centred form with a HalfNormal scale."""
    assert coef in ("var", "log", "derived_log")
    return _family(False, N, P, K, readers, (), coef, **kw)


def positions(model, count=3, seed=11):
    """Exact family: zero, then multiples of 1/8 in [-2, 2].  Real family: zero, then normal draws (scaled by 0.3, by 1)."""
    rng = np.random.default_rng([seed, model.n])
    if model.exact:
        return [np.zeros(model.n)] + [rng.integers(-16, 17, size=model.n) / 8.0 for _ in range(count - 1)]
    return [np.zeros(model.n)] + [rng.normal(size=model.n) * s for s in (0.3, 1.0)][: count - 1]


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@dataclass
class Exact:
    lik: Fraction                  # the factors' part of the log-density: exact
    logp: object                   # + the priors (mpmath, MP_PREC bits)
    grad: List[Fraction]           # d logp / d q: exact (the exact family), or of exp() at MP_PREC bits
    eta: List[object]              # per predictor: the exact eta [N, K] (`Dy`)
    loglik: Optional[object]       # per element of factor "y": sum_k -0.5 (y_k - eta_k)^2 (`Dy` [M])
    S_grad: np.ndarray             # per gradient element: the sum of the ABSOLUTE values of the terms it is made of (float64)
    S_logp: float                  # the same for the log-density

    def grad_floats(self):
        return np.array([float(g) for g in self.grad])

    def logp_float(self):
        return float(self.logp)


def _mp_exp(q):
    with mpmath.workprec(MP_PREC):
        return [mpmath.exp(mpmath.mpf(float(v))) for v in np.asarray(q).ravel()]


def evaluate_exact(model, q):
    """Log-density and gradient of `model` at the doubles q, without a rounding (exp: to MP_PREC bits)."""
    q = np.asarray(q, dtype="float64")
    big = not model.exact
    P, K, coef = model.P, model.K, model.coef
    D = lambda a: Dy.of(a, big)      # noqa: E731
    half_neg = D(np.array(-0.5))
    shrink = 1.0 - 2.0 ** -40        # (S is formed in float64: shrunk, so that a bound in terms of it is never wider than the true one)

    # coefficients B [P][K] of the constrained values, as exact numbers and as magnitudes
    if coef == "var":
        B = D(q.reshape(P, K))
    elif coef == "log":
        B = Dy.of_mpf(_mp_exp(q), (P, K))
    else:
        mu, z = D(q[0:1]), D(q[2:])
        T = D(q[1:2]) if coef == "derived" else Dy.of_mpf(_mp_exp(q[1:2]), (1,))
        B = (mu + T * z).reshape(P, 1)
    absB = np.abs(B.floats())

    gB, S_gB = None, np.zeros((P, K))
    lik, S_lik = Fraction(0), 0.0
    etas, loglik = [], None
    for l, X in enumerate(model.Xs):
        N = X.shape[0]
        Xd, absX = D(X), np.abs(X)
        eta = Xd @ B                                   # [N, K]
        S_eta = absX @ absB
        etas.append(eta)
        adj, S_adj = None, np.zeros((N, K))
        for r in (r for r in model.readers if r.pred == l):
            for j, k in enumerate(r.cols):
                ek = eta[:, k]                          # [N]
                if r.kind == "sq":
                    d = D(r.y[:, j]) - ek               # [M] (a one-row predictor broadcasts)
                    sq = d * d * half_neg
                    lik += sq.sum().fractions()[0]
                    if r.name == "y":
                        loglik = sq if loglik is None else loglik + sq
                    a = d if N > 1 else d.sum().reshape(1)
                    sa = np.abs(r.y[:, j]) + S_eta[:, k]
                    S_lik += 0.5 * float(np.sum(sa * sa))
                    sa = sa if N > 1 else np.array([sa.sum()])
                else:
                    w = D(np.array(r.w))
                    lik += ((ek * w).sum() * D(np.array(float(r.M if N == 1 else 1)))).fractions()[0]
                    a = D(np.full(N, r.w * (r.M if N == 1 else 1)))
                    sa = np.full(N, abs(r.w) * (r.M if N == 1 else 1))
                    S_lik += float(np.sum(abs(r.w) * S_eta[:, k])) * (r.M if N == 1 else 1)
                col = np.zeros((N, K))
                one = D(np.eye(K)[k][None, :])
                contrib = a.reshape(N, 1) * one         # the column's adjoint, in its place of [N, K]
                adj = contrib if adj is None else adj + contrib
                col[:, k] = sa
                S_adj += col
        if adj is not None:
            g = Xd.T @ adj                              # [P, K]
            gB = g if gB is None else gB + g
            S_gB += absX.T @ S_adj
    if gB is None:
        gB = D(np.zeros((P, K)))

    # back to the unconstrained variables, with the priors
    one = D(np.array(1.0))
    with mpmath.workprec(MP_PREC):
        log_sqrt_2pi = mpmath.log(2 * mpmath.pi) / 2
        half_log_2_pi = mpmath.log(2 / mpmath.pi) / 2

        def normal_lp(x):                               # sum of Normal(0, 1) log-densities of exact x
            return sum((mpmath.mpf(f.numerator) / f.denominator for f in (x * x * half_neg).fractions()), mpmath.mpf(0)) - x.m.size * log_sqrt_2pi

        def halfnormal_lp(b, qq):                       # HalfNormal(1) of b = exp(q) with the log transform's Jacobian
            s = sum((mpmath.mpf(f.numerator) / f.denominator for f in (b * b * half_neg).fractions()), mpmath.mpf(0))
            return s + b.m.size * half_log_2_pi + sum(mpmath.mpf(float(v)) for v in np.asarray(qq).ravel())

        if coef == "var":
            Bq = B.reshape(P * K)
            grad = (gB.reshape(P * K) - Bq).fractions()
            S_grad = S_gB.ravel() + np.abs(q)
            prior = normal_lp(Bq)
            S_prior = float(np.sum(0.5 * q * q)) + q.size * LOG_SQRT_2PI
        elif coef == "log":
            Bq, gq = B.reshape(P * K), gB.reshape(P * K)
            grad = (gq * Bq - Bq * Bq + one).fractions()
            b = absB.ravel()
            S_grad = S_gB.ravel() * b + b * b + 1.0
            prior = halfnormal_lp(Bq, q)
            S_prior = float(np.sum(0.5 * b * b) + np.sum(np.abs(q))) + q.size * abs(0.5 * math.log(2.0 / math.pi))
        else:
            gb = gB.reshape(P)
            gz_sum = (gb * z).sum().reshape(1)
            g_mu = gb.sum().reshape(1) - mu
            g_z = gb * T - z
            tf, zf, sg = float(abs(T.floats()[0])), np.abs(q[2:]), S_gB.ravel()
            if coef == "derived":
                g_tau = gz_sum - T
                S_tau = float(sg @ zf) + tf
                prior = normal_lp(D(q))
                S_prior = float(np.sum(0.5 * q * q)) + q.size * LOG_SQRT_2PI
            else:
                g_tau = gz_sum * T - T * T + one
                S_tau = float(sg @ zf) * tf + tf * tf + 1.0
                prior = normal_lp(mu) + normal_lp(z) + halfnormal_lp(T, q[1:2])
                S_prior = 0.5 * q[0] ** 2 + float(np.sum(0.5 * zf * zf)) + (P + 1) * LOG_SQRT_2PI + 0.5 * tf * tf + abs(q[1]) + abs(0.5 * math.log(2.0 / math.pi))
            grad = g_mu.fractions() + g_tau.fractions() + g_z.fractions()
            S_grad = np.concatenate([[float(sg.sum()) + abs(q[0])], [S_tau], sg * tf + zf])
        logp = mpmath.mpf(lik.numerator) / lik.denominator + prior
    return Exact(lik, logp, grad, etas, loglik, S_grad * shrink, (S_lik + S_prior) * shrink)


LOG_SQRT_2PI = 0.9189385332046727


def fraction_reference(model, q):
    """(lik, grad) of a `var` / `derived` model in plain `fractions.Fraction`, product by product (for small sizes)."""
    F = lambda v: Fraction(float(v))      # noqa: E731
    q = [F(v) for v in q]
    P, K = model.P, model.K
    if model.coef == "var":
        B = [[q[p * K + k] for k in range(K)] for p in range(P)]
    else:
        assert model.coef == "derived"
        B = [[q[0] + q[1] * q[2 + p]] for p in range(P)]
    gB = [[Fraction(0)] * K for _ in range(P)]
    lik = Fraction(0)
    for l, X in enumerate(model.Xs):
        N = X.shape[0]
        eta = [[sum((F(X[i, p]) * B[p][k] for p in range(P)), Fraction(0)) for k in range(K)] for i in range(N)]
        adj = [[Fraction(0)] * K for _ in range(N)]
        for r in (r for r in model.readers if r.pred == l):
            for j, k in enumerate(r.cols):
                for i in range(r.M):
                    row = i if N > 1 else 0
                    if r.kind == "sq":
                        d = F(r.y[i, j]) - eta[row][k]
                        lik += Fraction(-1, 2) * d * d
                        adj[row][k] += d
                    else:
                        lik += F(r.w) * eta[row][k]
                        adj[row][k] += F(r.w)
        for p in range(P):
            for k in range(K):
                gB[p][k] += sum((F(X[i, p]) * adj[i][k] for i in range(N)), Fraction(0))
    if model.coef == "var":
        return lik, [gB[p][k] - B[p][k] for p in range(P) for k in range(K)]
    gb = [gB[p][0] for p in range(P)]
    return lik, [sum(gb, Fraction(0)) - q[0], sum((g * z for g, z in zip(gb, q[2:])), Fraction(0)) - q[1]] + [q[1] * g - z for g, z in zip(gb, q[2:])]


# ---- the bound ----------------------------------------------------------------------------------------------------------------------
# Kernels B / C (pymc_amd/csrc/kernels.h) behind the node, as far as the counts below need them:
VEC_THREADS, EPT_MAX, CTL_CHUNKS, SWEEP_BLOCK = 256, 16, 8, 64


def _reduce_path(n_terms_per_thread, n_blocks):
    """Roundings on the longest path of a sum that kernel B starts and the control kernel finishes: a thread's own additions, the
    wave sum (6 DPP steps), the workgroup's 4 waves in order, `sum_strided` over a chunk of ceil(n_blocks / CTL_CHUNKS) per-workgroup
    records, the CTL_CHUNKS chunks in order, the control kernel's `block_sum` of its deferred elements (6 + 4) and the final addition."""
    return n_terms_per_thread + 6 + 4 + -(-n_blocks // CTL_CHUNKS) + CTL_CHUNKS + (6 + 4) + 1


def rounding_count(model):
    """C of |g_p - exact| <= C 2^-53 S_p, S_p = `Exact.S_grad`: the roundings on the LONGEST path from one product x_ip' b_p' to
    element p of the gradient, counted from pymc_amd/csrc/lin_kernel.h and its callers.  Every rounding acts on a partial sum whose
    magnitude is at most S_p (the sum of the absolute values of all the terms), so to first order the error is at most C 2^-53 S_p;
    `bound` adds the second-order part.  The largest count over the model's predictors and readers is taken.

      coefficient    0 a variable itself; 2 `exp` of a log-transformed one (`transform_x`: the device's exp, within 1 ulp, and the
                     true exp's own rounding); 2 + 2 `mu + exp(log_tau) z` (`k_derive`: exp, the product, the addition)
      forward        N > 1: P fmas in column order (`k_lin_fwd`)
                     N = 1: ceil(P / 1024) fmas of a thread, the wave sum (6), the 16 waves in order (`k_lin_fwd1`, `block_sum`)
      adjoint        1: y - eta (the sweep; the factors -0.5, 2 and -1 of the square's reverse pass are exact)
                     + (readers - 1): `lin_adj` adds the reading factors' adjoints in order
      backward       N > 1: 8 fmas of a thread over its LIN_CHUNK / 256 rows, the wave sum (6), the 4 waves (`k_lin_bwd`), then
                     `sum_strided` over the nchunk chunk partials and the n_src additions of `k_lin_fin`
                     N = 1: sum over the readers of ceil(M / 1024) additions of a thread, 6 + 16 (`k_lin_bwd1`), then x_p * total and
                     the n_src additions (`k_lin_fin`)
      kernels B / C  the prior's share -(x - mu) / sigma^2 (3), gx + lin_gdense (1), (.) * dxdq + dj (2), dxdq = exp(q) (2 where
                     the variable is log-transformed)
      derived        the seed of element p goes back through `mu + tau z_p`: tau * seed (1) for z; for the SCALARS mu and tau the P
                     seeds (times z_p: 1) are added up by kernel B and the control kernel: `_reduce_path` with EPT_MAX elements per
                     thread; times dxdq = tau (1)
    """
    P = model.P
    coef_r = {"var": 0, "log": 2, "derived": 2, "derived_log": 4}[model.coef]
    n_src = len(model.Xs)
    worst = 0
    for l, X in enumerate(model.Xs):
        N = X.shape[0]
        rs = [r for r in model.readers if r.pred == l]
        n_use = max([sum(1 for r in rs if k in r.cols) for k in range(model.K)] + [1])
        if N > 1:
            fwd = P
            bwd = 8 + 6 + 4 + -(-N // LIN_CHUNK) + n_src
        else:
            fwd = -(-P // 1024) + 6 + 16
            bwd = sum(-(-r.M // 1024) for r in rs) + 6 + 16 + 1 + n_src
        worst = max(worst, coef_r + fwd + 1 + (n_use - 1) + bwd)
    tail = 3 + 1 + 2 + (2 if model.coef in ("log", "derived_log") else 0)
    if model.coef in ("derived", "derived_log"):
        nblk = -(-model.n // VEC_THREADS)
        tail += 1 + 1 + _reduce_path(EPT_MAX, nblk) + 1
    return worst + tail


def logp_rounding_count(model):
    """C of |logp - exact| <= C 2^-53 S, S = `Exact.S_logp`: the longest path from one term to the log-density.  In the exact
    family the factors' part is exact however it is grouped; roundings begin where a PRIOR term (inexact: -0.5 x^2 - log sqrt(2 pi))
    meets it, and from there on every addition may round a sum of magnitude at most S.

      a term         real family: the error of eta relative to sum |x b| (coefficient + forward counts of `rounding_count`) and of
                     y - eta (1) enters the square twice; the square and the adjoining additions of the factor's program: 2 + K
                     exact family: 0 (the factors' part is exact)
                     a prior's element: (x - mu) / sigma (2), -0.5 z z (1), the two constants and their own representation (4);
                     exp and the Jacobian of a log-transformed variable (3)
      the sweep      a workgroup's sum of its SWEEP_BLOCK elements: 6 + 1 (`k_gsweep_fast`: one wave; the generic sweeps have 4)  -> 10
      kernel B       workgroup 0 adds the sweep's records to its threads' own sums: ceil(records / VEC_THREADS) additions each, after
                     at most 2 EPT_MAX additions for the thread's own elements (Jacobian and density); records <= elements / SWEEP_BLOCK
                     + one per factor
      then           `_reduce_path` over the ceil(n / VEC_THREADS) workgroups (kernel B's grid is never larger)
    """
    elems = sum(r.M for r in model.readers)
    records = -(-elems // SWEEP_BLOCK) + len(model.readers)
    per_thread = 2 * EPT_MAX + -(-records // VEC_THREADS)
    term = 7 + 3
    if not model.exact:
        coef_r = {"var": 0, "log": 2, "derived": 2, "derived_log": 4}[model.coef]
        fwd = max(model.P if X.shape[0] > 1 else -(-model.P // 1024) + 22 for X in model.Xs)
        term = max(term, 2 * (coef_r + fwd + 1) + 2 + model.K)
    return term + 10 + _reduce_path(per_thread, -(-model.n // VEC_THREADS))


def bound(C, S):
    """C 2^-53 S with its second-order part: (1 + 2^-53)^C - 1 <= C 2^-53 (1 + 2^-30) at C < 2^22."""
    assert C < 1 << 22
    return C * U * S * (1.0 + 2.0 ** -30)


# ---- the cases the device runs (tests/test_gpu_lin_edges.py) and the host holds the references of (tests/test_lin_edges.py) -----------
def _cases():
    c = {}
    for N in (2, 255, 256, 257, 2047, 2048, 2049, 4096, 4097):       # workgroup edges of the forward pass, chunk edges of the backward pass
        c[f"rows-N{N}"] = dict(N=N, P=5)
    c["grid-stride-N1048833"] = dict(N=FWD_MAX_GRID * FWD_THREADS + 257, P=1)      # a second trip of the forward pass, 513 backward chunks
    for K in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16):                           # every KT, full and partly filled
        c[f"cols-K{K}"] = dict(N=300, P=6, K=K)
    for P in (1, 2, 3, 4, 7, 8, 511, 512):                               # the four-column step of the forward pass and its remainder; NUTS_LIN_MAXP
        c[f"width-P{P}"] = dict(N=300, P=P)
    c["limit-P512-K8"] = dict(N=2049, P=512, K=8)                        # K P = 4096: 32 KB of coefficients in LDS, a backward grid of 2 x 512
    c["limit-P256-K16"] = dict(N=300, P=256, K=16)
    for r in (2, 3, 4):                                                  # `lin_adj`, up to LIN_MAXUSE
        c[f"readers-{r}"] = dict(N=2049, P=3, K=5, readers=r)
    c["readers-2-some-columns"] = dict(N=2049, P=3, K=5, readers=2, reader_cols=(1, 3))
    c["derived-N2049-P7"] = dict(N=2049, P=7, coef="derived")
    c["derived-N300-P512"] = dict(N=300, P=512, coef="derived")
    c["shared-coefficients"] = dict(N=300, P=5, N2=2049)                 # one vector against two matrices: LinTarget.n_src = 2
    for P in (1, 1023, 1024, 1025, 8191, 8192, 8193, 9217):              # one-row predictors: a trip of 8 x 1024, full, short, and a second
        c[f"one-row-P{P}"] = dict(N=1, P=P, M=7)
    for M in (1, 1025, 8192, 8193):                                      # ... broadcast into a factor of M elements
        c[f"one-row-M{M}"] = dict(N=1, P=1025, M=M)
    c["one-row-two-readers"] = dict(N=1, P=1025, M=1025, M2=8193, readers=2)
    return c


EXACT_CASES = _cases()
UNREAD_CASE = dict(N=300, P=6, K=3, unread=(2,))       # column 2 is read by no factor (after the fix: `lin_adj` skips it)
ROUTE_CASES = ("rows-N2049", "cols-K5", "readers-3", "one-row-P8193")
LOGLIK_CASES = ("rows-N257", "loglik-N2049-K5", "grid-stride-N1048833")
EXACT_CASES["loglik-N2049-K5"] = dict(N=2049, P=3, K=5)
REAL_CASES = {
    "real-N2049-P7-noncentred": dict(N=2049, P=7, coef="derived_log"),
    "real-N300-P512-K8-log": dict(N=300, P=512, K=8, coef="log"),
    "real-one-row-P9217": dict(N=1, P=9217, M=7),
}
NUTS_CASE = dict(N=300, P=4, K=2, readers=2)


@functools.lru_cache(maxsize=None)
def exact_case(name):
    return exact_model(**(UNREAD_CASE if name == "unread-column" else EXACT_CASES[name]))


@functools.lru_cache(maxsize=None)
def real_case(name):
    return real_model(**REAL_CASES[name])


@functools.lru_cache(maxsize=None)
def reference(kind, name):
    """[(q, Exact)] at the case's three positions: computed once, shared, left unchanged."""
    model = exact_case(name) if kind == "exact" else real_case(name)
    return tuple((q, evaluate_exact(model, q)) for q in positions(model))


def deterministic_model(n_unread=4):
    """The model of tests/test_lin_node.py `test_deterministics_over_a_predictor_are_evaluated_on_the_host`: two predictors, the
    first read only by a Deterministic (`n_unread` rows), the second by the likelihood (4 rows)."""
    from pymc_amd.model_spec import ModelBuilder

    m = ModelBuilder()
    X = np.arange(12.0).reshape(4, 3)
    Xu = X[:n_unread] + 1.0
    b = m.Normal("b", 0.0, 1.0, shape=3)
    m.Deterministic("eta2", m.dot(Xu, b) * 2.0)
    m.Normal("y", mu=m.dot(X, b), sigma=1.0, observed=np.zeros(4))
    return m.build(), X, Xu


def first_wrong(got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return int(bad[0]) if bad.size else None


def gradient_message(model, got, want):
    """Which coefficient is wrong, for an exact model (names the column and the coefficient)."""
    i = first_wrong(got, want)
    if i is None:
        return ""
    if model.coef == "var":
        p, k = divmod(i, model.K)
        what = f"coefficient p = {p} of column k = {k} (KT = {kt_of(model.K)})"
    else:
        what = ["mu", "tau"][i] if i < 2 else f"z[{i - 2}]"
    return f"{model.label}: gradient element {i} ({what}): device {got[i]!r}, exact {want[i]!r}, difference {got[i] - want[i]!r}; {int(np.sum(got != want))} of {len(want)} wrong"
