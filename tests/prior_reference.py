"""NumPy restatement of the prior draws (pymc_amd/csrc/prior.h, csrc/prior_kernel.h) on top of the restatement of the variates
(tests/predictive_reference.py, imported and not edited):

  the address            counter = (i low, i high | 0x80000000, s, index << 16 | t) under key = (seed low, seed high): the element
                         index with bit 63 set, which no observation index has
  the forward transforms log(x); log(x) - log1p(-x); the same of (x - lower) / (upper - lower); x
  the Dirichlet draw     g_k = gamma(alpha_k) at element k, w = g / sum g (index order), y = log w, y[:-1] - mean(y)
                         (`SimplexTransform.forward`, pymc/logprob/transforms.py:1091-1100)
  the sampler            level by level over `predictive.prior_plan`: a factor's arguments from `model_spec.eval_program` at the
                         constrained values of the parents, the variate of its family, the forward transform

The gamma generator is restated once more here WITH its acceptance margin (the smallest distance by which an attempt's accept /
reject decision was taken): an implementation whose libm rounds differently may decide an attempt with a tiny margin the other
way, and then draws a different value.  Every result of `draw` / `dirichlet` / `sample` comes with that margin (+inf for the
families without a rejection loop).
"""
import numpy as np

import predictive_reference as ref
from pymc_amd import model_spec as ms
from pymc_amd import predictive, trace

BIT63 = 1 << 63
GAMMA_FAMILIES = (ref.D_GAMMA, ref.D_INVGAMMA, ref.D_BETA, ref.D_STUDENTT)


class Address(ref.Address):
    """(seed, variable index, draws s, elements i) of a PRIOR variate"""

    def __init__(self, seed, index, s, i):
        super().__init__(seed, 0, index, s, np.asarray(i, dtype=np.uint64) | np.uint64(BIT63))


def forward(var, x):
    """untransformed variable -> value variable (the inverse of `trace.backward`, element-wise transforms)"""
    x = np.asarray(x, dtype="float64")
    with np.errstate(divide="ignore", invalid="ignore"):
        if var.transform == ms.TR_LOG:
            return np.log(x)
        if var.transform == ms.TR_LOGODDS:
            return np.log(x) - np.log1p(-x)
        if var.transform == ms.TR_INTERVAL:
            p = (x - var.lower) / (var.upper - var.lower)
            return np.log(p) - np.log1p(-p)
    return x


def gamma(a, adr, t0):
    """`ref.gamma` with the margin of its decisions -> (g, margin)"""
    a = np.broadcast_to(np.asarray(a, dtype="float64"), adr.shape)
    out = np.full(adr.shape, np.nan)
    margin = np.full(adr.shape, np.inf)
    todo = np.ones(adr.shape, dtype=bool)
    a1 = np.where(a < 1.0, a + 1.0, a)
    d = a1 - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    for j in range(ref.GAMMA_TRIES):
        if not todo.any():
            break
        sub = adr.sub(todo)
        x = sub.normal(t0 + 2 * j)
        u, u2 = sub.block(t0 + 2 * j + 1)
        dd, aa = d[todo], a[todo]
        w = 1.0 + c[todo] * x
        v = w * w * w
        with np.errstate(invalid="ignore", divide="ignore"):
            lhs, rhs = np.log(u), 0.5 * x * x + dd - dd * v + dd * np.log(v)
            ok = (v > 0.0) & (lhs < rhs)
            mg = np.where(v > 0.0, np.minimum(np.abs(w), np.abs(lhs - rhs)), np.abs(w))      # (v > 0 is decided by w = 1 + c x)
            g = dd * v
            g = np.where(aa < 1.0, g * np.exp(np.log(u2) / aa), g)
        idx = np.flatnonzero(todo.ravel())
        margin.ravel()[idx] = np.minimum(margin.ravel()[idx], mg)
        out.ravel()[idx[ok]] = g[ok]
        todo.ravel()[idx[ok]] = False
    return out, margin


def draw(dist, a1, a2, a3, adr):
    """`ref.draw` for the continuous families -> (values, acceptance margin)"""
    if dist not in GAMMA_FAMILIES:
        return ref.draw(dist, a1, a2, a3, adr)
    a1, a2, a3 = (np.broadcast_to(np.asarray(a, dtype="float64"), adr.shape) for a in (a1, a2, a3))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if dist == ref.D_GAMMA:
            be = 1.0 / (1.0 / a2)
            ok = (a1 > 0) & (be > 0)
            g, m = gamma(np.where(ok, a1, 1.0), adr, 0)
            return np.where(ok, g / be, np.nan), np.where(ok, m, np.inf)
        if dist == ref.D_INVGAMMA:
            ok = (a1 > 0) & (a2 > 0)
            g, m = gamma(np.where(ok, a1, 1.0), adr, 0)
            return np.where(ok, a2 / g, np.nan), np.where(ok, m, np.inf)
        if dist == ref.D_BETA:
            ok = (a1 > 0) & (a2 > 0)
            (g1, m1), (g2, m2) = gamma(np.where(ok, a1, 1.0), adr, 0), gamma(np.where(ok, a2, 1.0), adr, 2 * ref.GAMMA_TRIES)
            return np.where(ok, g1 / (g1 + g2), np.nan), np.where(ok, np.minimum(m1, m2), np.inf)
        ok = (a1 > 0) & (a3 > 0)
        nu = np.where(ok, a1, 1.0)
        g, m = gamma(0.5 * nu, adr, 0)
        return np.where(ok, a2 + a3 * adr.normal(ref.T_BLOCK) / np.sqrt(2.0 * g / nu), np.nan), np.where(ok, m, np.inf)


def dirichlet(alpha, seed, index, s):
    """-> (y [S, K - 1] the simplex-transformed value, w [S, K], margin [S]) of draws `s` of variable `index`"""
    alpha = np.asarray(alpha, dtype="float64")
    K = alpha.size
    s = np.atleast_1d(np.asarray(s))
    g, m = gamma(np.broadcast_to(alpha, (s.size, K)), Address(seed, index, s[:, None], np.arange(K)[None, :]), 0)
    total = np.zeros(s.size)
    for k in range(K):          # (index order, as the header adds them)
        total = total + g[:, k]
    w = g / total[:, None]
    ly = np.log(w)
    lsum = np.zeros(s.size)
    for k in range(K):
        lsum = lsum + ly[:, k]
    return ly[:, :-1] - (lsum / K)[:, None], w, m.min(axis=1)


def constrained(spec, q):
    """q [S, n] -> the constrained values in the spec's layout (a simplex variable keeps its stored values: no factor reads it)"""
    x = np.empty_like(q)
    with np.errstate(all="ignore"):
        for v in spec.vars:
            blk = q[:, v.offset : v.offset + v.size]
            x[:, v.offset : v.offset + v.size] = blk if getattr(v, "simplex", False) else trace.backward(v, blk)
    return x


def factor_args(spec, fi, x):
    """arguments 1 .. 3 of factor `fi` at the constrained values x [S, n], each broadcast to [S, size]"""
    f = spec.factors[fi]
    out = []
    for j in (1, 2, 3):
        a = ms.eval_program(spec, f.prog, f.args[j], x) if j < len(f.args) else np.zeros(())
        out.append(np.broadcast_to(a, (x.shape[0], f.size)))
    return out


def sample(spec, S, seed, draw0=0, given=None):
    """S prior draws numbered draw0 .. -> (q [S, n], margin [S, n]).  `given` (q of another implementation, [S, n]): every level is
    drawn given THAT implementation's values of the earlier levels, so one element decided the other way does not compound."""
    by_name = {v.name: k for k, v in enumerate(spec.vars)}
    q = np.zeros((S, spec.n))
    margin = np.full((S, spec.n), np.inf)
    s = draw0 + np.arange(S)
    for level in predictive.prior_plan(spec):
        x = constrained(spec, q if given is None else given)
        for name, fi in level:
            k = by_name[name]
            v = spec.vars[k]
            sl = slice(v.offset, v.offset + v.size)
            if fi < 0:
                q[:, sl], _, m = dirichlet(spec.mixture_rows.w_alpha, seed, k, s)
                margin[:, sl] = m[:, None]
                continue
            a1, a2, a3 = factor_args(spec, fi, x)
            val, m = draw(spec.factors[fi].dist, a1, a2, a3, Address(seed, k, s[:, None], np.arange(v.size)[None, :]))
            q[:, sl], margin[:, sl] = forward(v, val), m
    return q, margin
