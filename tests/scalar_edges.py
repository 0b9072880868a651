"""Scalar ops of the expression programs at the edges of their domains: point tables, mpmath truths, the error measure, the regime
table with the oracle's own error, and the builders of the isolating models.  A plain helper module (imported explicitly by
tests/test_scalar_edges.py on the host and tests/test_gpu_scalar_edges.py on the device).

The measure.  For a result `a` with truth T at exact double inputs x, y, ...:

    e(a) = |a - T| / ( ulp(T) + ulp(x) |dT/dx| + ulp(y) |dT/dy| + ... )

forward error in ulps of the result plus what one ulp of each input may move it; T and its partials come from mpmath at 2000 bits
(every truth is recomputed at 4000 bits and must round to the same double).  The same measure is applied to every derivative an
op's reverse rule produces, with the truth's second partials in the denominator.

Regimes.  A regime is a stretch of one op's domain served by one code branch, or one where the reference's own formula cancels.
A regime's error is the maximum of e over its points.  `E_O` below is the oracle's (oracle/ref_models.py `_instr_value`) error on
the regime's points, asserted by tests/test_scalar_edges.py; the device must stay within 16 max(1, E_O): 16 ulp is the loosest
error the OpenCL C accuracy table grants a single double-precision library call (erf, erfc, pow, lgamma), the table the ROCm
device library is built to.

Isolation.  `Potential(s * op(x))` over Flat vectors evaluated at s = 1: grad[s_i] is op(x_i) and grad[x_i] is op'(x_i), element by
element with no sum in between.
"""
import functools
import math

import mpmath as mp
import numpy as np

from oracle import ref_models as rm
from pymc_amd.model_spec import ModelBuilder

PREC = 2000
FACTOR = 16.0
LOG2 = math.log(2.0)
DIGAMMA_ROOT = 1.4616321449683623
DIGAMMA_NEG_ROOT = -0.504083008264455
TINY = 5e-324


def near(*vals):
    """every listed value with its two neighbouring doubles"""
    out = []
    for v in vals:
        for w in (np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)):
            if float(w) not in out:
                out.append(float(w))
    return out


def _pm(vals):
    return [s * v for v in vals for s in (1.0, -1.0)]


# ---- point tables (one row per point, one column per operand) -------------------------------------------------------------------
_GAMMA_SMALL = [1e-300, 1e-8, 0.25, 0.5 - 1e-6, 0.5 + 1e-6, 1.0, 1.46, DIGAMMA_ROOT, 2.0, 10.0 - 1e-6, 10.0 + 1e-6, 50.0, 1e3, 1e8, 1e15, 1e300]
_GAMMA_NEG = [-1e-8, -0.25, -0.5, -0.999, -1.0 - 1e-6, -1.0 + 1e-6, -1.0 + 1e-9, -1.5, -2.5, -10.3, -100.25, -1000.7, -1e6 - 0.5, DIGAMMA_NEG_ROOT]
_ERF = [-26.0, -10.0, -5.0, -1.0, -1e-8, 1e-8, 0.0, 0.5, 1.0, 5.0, 10.0, 26.0, 27.0, 50.0, 1e3, 1e4, 1e8, 1e150]
_SOFT = [800.0, -800.0, 745.0, -745.0, 709.0, -709.0, -37.0 - 1e-6, -37.0 + 1e-6, 0.0, 1.0, -1.0, 18.0 - 1e-6, 18.0 + 1e-6, 33.3 - 1e-6, 33.3 + 1e-6, 100.0,
         -50.0, -20.0, -5.0, 5.0, 10.0, 25.0]      # (the last six: the middle of every branch, where a moved threshold shows)


def _col(vals):
    return np.asarray(vals, dtype="d").reshape(-1, 1)


def _logaddexp_points():
    d = near(*_SOFT)
    return np.asarray([(v, 0.0) for v in d] + [(0.25 + v, 0.25) for v in d] + [(-3.5, -3.5 - v) for v in _SOFT], dtype="d")


def _pow_points():
    pts = [(x, y) for x in (TINY, 1e-300, 1e-8) for y in (1.0, 0.5, 1e-8, -1e-8, -0.5)]
    pts += [(x, y) for x in (np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)) for y in (1e15, -1e15, 2.0 ** 52, 1e17, -1e17)]
    pts += [(2.0, 0.5), (10.0, -3.0), (0.5, 100.0), (3.0, 3.0), (1e300, 1.0), (1e-300, 1.0), (7.5, 0.0)]
    return np.asarray(pts, dtype="d")


POINTS = {
    "digamma": _col(near(*_GAMMA_SMALL, *_GAMMA_NEG)),
    "gammaln": _col(near(*_GAMMA_SMALL, *_GAMMA_NEG, 1.0 - 1e-6, 1.0 + 1e-6, 2.0 - 1e-6, 2.0 + 1e-6, 171.5)),
    "erf": _col(near(*_ERF)),
    "erfc": _col(near(*_ERF)),
    "erfcx": _col(near(*_ERF)),
    "log1mexp": _col(near(-1e-300, -1e-16, -1e-8, -0.1, -LOG2, -1.0, -10.0, -37.0, -40.0, -700.0, -745.0)),
    "softplus": _col(near(*_SOFT)),
    "sigmoid": _col(near(*_SOFT)),
    "logaddexp": _logaddexp_points(),
    "expm1": _col(near(*_pm([1e-300, 1e-8, 1.0, 40.0]), -745.0, 700.0, 0.0)),
    "log1p": _col([-1.0 + 2.0 ** -53, -1.0 + 2.0 ** -52] + near(-0.5, 0.0, *_pm([1e-300, 1e-8]), 1.0, 1e8, 1e300)),
    "tanh": _col(near(0.0, *_pm([1e-300, 1e-8, 0.5, 1.0, 19.0, 40.0, 800.0]))),
    "pow": _pow_points(),
    "log": _col(near(1.0, 1.0 - 1e-8, 1.0 + 1e-8, 0.5, 2.0, 1e300) + [TINY, 2 * TINY, 1e-300]),
    "sqrt": _col([TINY, 2 * TINY, 1e-310] + near(2.2250738585072014e-308, 1.0, 2.0, 1e300)),
    "reciprocal": _col(near(1e-150, 1.0, 3.0, 1e150, 1e300) + [1.7e308, -1.7e308, -3.0]),
    "exp": _col(near(-745.0, -709.0, -1.0, 0.0, 1.0, 700.0)),
    "div": np.asarray([(1.0, 3.0), (-7.0, 1e-8), (1e-300, 3.0), (TINY, 2.0), (1e300, -1e5), (2.0, 1e300), (0.0, 5.0)], dtype="d"),
    "maximum": np.asarray([(1.0, 2.0), (2.0, 1.0), (-0.5, -0.5), (1e300, -1e300), (-TINY, 0.0), (3.0, np.nextafter(3.0, 4.0))], dtype="d"),
    "minimum": np.asarray([(1.0, 2.0), (2.0, 1.0), (-0.5, -0.5), (1e300, -1e300), (-TINY, 0.0), (3.0, np.nextafter(3.0, 4.0))], dtype="d"),
    "clip": np.asarray([(-1.0, -0.7, 1.3), (0.3, -0.7, 1.3), (2.0, -0.7, 1.3), (-0.7, -0.7, 1.3), (1.3, -0.7, 1.3), (1e300, -1e300, 1e299)], dtype="d"),
    "switch": np.asarray([(0.0, 1.5, -2.5), (1.0, 1.5, -2.5), (-2.5, 1e300, 3.0), (TINY, 4.0, 1e-300), (-0.0, 7.0, 8.0)], dtype="d"),
}

# Points where the truth or the oracle is not finite: class agreement only (tests "conventions"), never in an accuracy model.  The
# points of POINTS whose value or one of whose derivatives is not a finite double (trigamma at 1e-300, d erfcx at -26 ...) join
# them automatically (`split_points`).  digamma / gammaln: never an exact non-positive integer (scalar_math.h: the pole convention
# is not SciPy's).
CONVENTION_POINTS = {
    "log": _col([0.0, -1.0]),
    "log1p": _col([-1.0, -2.0]),
    "sqrt": _col([0.0, -1.0]),
    "reciprocal": _col([0.0, TINY, 1e-310, 1e-300]),
    "log1mexp": _col([0.0, 1.0]),
    "erfcx": _col([-27.0, -50.0]),
    "expm1": _col([710.0, 1e300]),
    "exp": _col([710.0, 1e300]),
    "softplus": _col([1e300, -1e300]),
    "gammaln": _col([1e306, 1e308]),
    "pow": np.asarray([(0.0, 0.5), (0.0, 0.0), (0.0, -1.0), (0.0, 2.0), (0.0, 1.0), (-1.0, 0.5), (TINY, -1.0), (1e300, 2.0)], dtype="d"),
    "div": np.asarray([(1.0, 0.0), (0.0, 0.0), (-1.0, 0.0), (1e300, 1e-300)], dtype="d"),
}

OPCODE = {"digamma": rm.E_DIGAMMA, "gammaln": rm.E_GAMMALN, "erf": rm.E_ERF, "erfc": rm.E_ERFC, "erfcx": rm.E_ERFCX, "log1mexp": rm.E_LOG1MEXP,
          "softplus": rm.E_SOFTPLUS, "sigmoid": rm.E_SIGMOID, "logaddexp": rm.E_LOGADDEXP, "expm1": rm.E_EXPM1, "log1p": rm.E_LOG1P,
          "tanh": rm.E_TANH, "pow": rm.E_POW, "log": rm.E_LOG, "sqrt": rm.E_SQRT, "reciprocal": rm.E_RECIPROCAL, "exp": rm.E_EXP,
          "div": rm.E_DIV, "maximum": rm.E_MAXIMUM, "minimum": rm.E_MINIMUM, "clip": rm.E_CLIP, "switch": rm.E_SWITCH}
OUTPUTS = ("v", "dx", "dy", "dz")


def arity(op):
    return POINTS[op].shape[1]


# ---- mpmath truths: (T, [dT/dx_k], [[d2T/dx_j dx_k]]) in forms that do not cancel -----------------------------------------------
def _erfcx_mp(x):
    if x < 1000:
        return mp.exp(x * x) * mp.erfc(x)
    # asymptotic series 1/(x sqrt pi) sum (-1)^n (2n-1)!! / (2 x^2)^n: at x >= 1e3 its terms fall by 1e-6 each, down to 2^-prec
    t, s, n, h = mp.mpf(1), mp.mpf(1), 0, 1 / (2 * x * x)
    while abs(t) > mp.ldexp(1, -mp.mp.prec - 10):
        n += 1
        t = -t * (2 * n - 1) * h
        s += t
    return s / (x * mp.sqrt(mp.pi))


def _sig(x):
    return 1 / (1 + mp.exp(-x))


@functools.lru_cache(maxsize=None)
def _gamma_family(xf, prec):
    """(log|Gamma|, psi, psi', psi'')(xf) at `prec` bits: reflection below 0, recurrence up to X = prec / 6 + 10, then Stirling's series
    and its derivatives (smallest term about exp(-2 pi X) < 2^-prec).  mpmath's own polygamma goes through the Hurwitz zeta function
    and takes minutes at this precision; tests/test_scalar_edges.py holds this restatement to mpmath's functions at 200 bits."""
    with mp.workprec(prec):
        x = mp.mpf(xf)
        if x < 0:
            lg, p0, p1, p2 = _gamma_family_pos(1 - x)
            px = mp.pi * x
            sn = mp.sin(px)
            cot, csc2 = mp.cos(px) / sn, 1 / (sn * sn)
            return mp.log(mp.pi / abs(sn)) - lg, p0 - mp.pi * cot, mp.pi ** 2 * csc2 - p1, p2 - 2 * mp.pi ** 3 * csc2 * cot
        return _gamma_family_pos(x)


def _gamma_family_pos(x):
    r0 = r1 = r2 = mp.mpf(0)
    prod = mp.mpf(1)
    big = mp.mpf(mp.mp.prec // 6 + 10)
    while x < big:
        i = 1 / x
        prod *= x
        r0 -= i
        r1 += i * i
        r2 -= 2 * i * i * i
        x += 1
    i = 1 / x
    i2, eps = i * i, mp.ldexp(1, -mp.mp.prec - 40)
    lx = mp.log(x)
    sl, s0, s1, s2 = (x - mp.mpf(0.5)) * lx - x + mp.log(2 * mp.pi) / 2, lx - i / 2, i + i2 / 2, -i2 - i2 * i
    p, k = i2, 1          # p = x^-2k
    while True:
        u = mp.bernoulli(2 * k) * p
        t0 = u / (2 * k)
        t1 = u * i
        t2 = t1 * i * (2 * k + 1)
        sl, s0, s1, s2 = sl + t0 * x / (2 * k - 1), s0 - t0, s1 + t1, s2 - t2
        if abs(t2) < eps * abs(s2):          # (relative to its sum the largest of the four terms)
            break
        p, k = p * i2, k + 1
        assert k < 4000
    return sl - mp.log(prod), r0 + s0, r1 + s1, r2 + s2


def gamma_family(x):
    return _gamma_family(float(x), mp.mp.prec)


def _sig1(x):          # s (1 - s)
    return 1 / ((1 + mp.exp(-x)) * (1 + mp.exp(x)))


def _unary(op, x):
    two_rpi = 2 / mp.sqrt(mp.pi)
    if op == "digamma":
        return gamma_family(x)[1:]
    if op == "gammaln":
        return gamma_family(x)[:3]
    if op == "erf":
        g = two_rpi * mp.exp(-x * x)
        return mp.erf(x), g, -2 * x * g
    if op == "erfc":
        g = two_rpi * mp.exp(-x * x)
        return mp.erfc(x), -g, 2 * x * g
    if op == "erfcx":
        v = _erfcx_mp(x)
        d = 2 * x * v - two_rpi
        return v, d, 2 * v + 2 * x * d
    if op == "log1mexp":
        u = mp.expm1(-x)
        return (mp.log(-mp.expm1(x)) if x > -1 else mp.log1p(-mp.exp(x))), -1 / u, -mp.exp(-x) / (u * u)
    if op == "softplus":
        return mp.log1p(mp.exp(x)), _sig(x), _sig1(x)
    if op == "sigmoid":
        return _sig(x), _sig1(x), -_sig1(x) * mp.tanh(x / 2)
    if op == "expm1":
        return mp.expm1(x), mp.exp(x), mp.exp(x)
    if op == "exp":
        return mp.exp(x), mp.exp(x), mp.exp(x)
    if op == "log1p":
        return mp.log1p(x), 1 / (1 + x), -1 / ((1 + x) * (1 + x))
    if op == "tanh":
        c = mp.cosh(x)
        return mp.tanh(x), 1 / (c * c), -2 * mp.tanh(x) / (c * c)
    if op == "log":
        return mp.log(x), 1 / x, -1 / (x * x)
    if op == "sqrt":
        r = mp.sqrt(x)
        return r, 1 / (2 * r), -1 / (4 * r * x)
    if op == "reciprocal":
        return 1 / x, -1 / (x * x), 2 / (x * x * x)
    raise KeyError(op)


def _truth_mp(op, p):
    """p: tuple of mpf operands -> (T, grad list, hessian rows)"""
    zero, one = mp.mpf(0), mp.mpf(1)
    if len(p) == 1:
        t, d1, d2 = _unary(op, p[0])
        return t, [d1], [[d2]]
    if op == "logaddexp":
        x, y = p
        d = x - y
        t = (x if d > 0 else y) + mp.log1p(mp.exp(-abs(d)))
        q = _sig1(d)
        return t, [_sig(d), _sig(-d)], [[q, -q], [-q, q]]
    if op == "pow":
        x, y = p
        t, lx = mp.power(x, y), mp.log(x)
        xy1 = mp.power(x, y - 1)
        m = xy1 * (1 + y * lx)
        return t, [y * xy1, t * lx], [[y * (y - 1) * mp.power(x, y - 2), m], [m, t * lx * lx]]
    if op == "div":
        x, y = p
        return x / y, [1 / y, -x / (y * y)], [[zero, -1 / (y * y)], [-1 / (y * y), 2 * x / (y * y * y)]]
    if op in ("maximum", "minimum"):     # the reference's convention: every operand equal to the result receives the adjoint
        x, y = p
        t = max(x, y) if op == "maximum" else min(x, y)
        return t, [one if t == x else zero, one if t == y else zero], [[zero, zero], [zero, zero]]
    z3 = [[zero] * 3] * 3
    if op == "clip":
        x, lo, hi = p
        if x < lo:
            return lo, [zero, one, zero], z3
        if x > hi:
            return hi, [zero, zero, one], z3
        return x, [one, zero, zero], z3
    if op == "switch":
        c, y, z = p
        return (y, [zero, one, zero], z3) if c != 0 else (z, [zero, zero, one], z3)
    raise KeyError(op)


def _to_double(v):
    try:
        return float(v)
    except OverflowError:
        return math.inf if v > 0 else -math.inf


def _truth_at(op, pt, prec):
    with mp.workprec(prec):
        return _truth_mp(op, tuple(mp.mpf(float(c)) for c in pt))


@functools.lru_cache(maxsize=None)
def truths(op, convention=False):
    """[(T, grad, hess)] of every point of the op's table, in mpf at PREC bits; asserts that doubling the precision returns the
    same doubles."""
    out = []
    for pt in (CONVENTION_POINTS if convention else POINTS)[op]:
        try:
            a, b = _truth_at(op, pt, PREC), _truth_at(op, pt, 2 * PREC)
        except (ValueError, ZeroDivisionError, TypeError):
            assert convention, (op, pt)
            out.append(None)          # outside the domain (log(0), a pole ...): no truth
            continue
        if not convention:
            fa = [_to_double(a[0])] + [_to_double(g) for g in a[1]]
            fb = [_to_double(b[0])] + [_to_double(g) for g in b[1]]
            assert fa == fb, (op, pt, fa, fb)
        out.append(a)
    return out


def ulp(v):
    v = abs(float(v))
    return float(np.spacing(v)) if math.isfinite(v) else math.inf


def measure(a, t, sens, pt):
    """e(a) of the module docstring; `t` mpf truth, `sens` its partials w.r.t. the operands `pt`."""
    if not math.isfinite(a):
        return math.inf
    with mp.workprec(PREC):
        den = mp.mpf(ulp(_to_double(t)))
        for s, x in zip(sens, pt):
            den += mp.mpf(ulp(x)) * abs(s)
        return float(abs(mp.mpf(float(a)) - t) / den)


def oracle_outputs(op, pts):
    """{output: array} of oracle/ref_models.py `_instr_value` at the points"""
    cols = [np.ascontiguousarray(pts[:, k]) for k in range(pts.shape[1])] + [None] * (3 - pts.shape[1])
    with np.errstate(all="ignore"):
        r = rm._instr_value(OPCODE[op], 0.0, cols[0], cols[1], cols[2])
    out = {}
    for name, v in zip(OUTPUTS[: 1 + pts.shape[1]], r):
        out[name] = np.zeros(len(pts)) if v is None else np.broadcast_to(np.asarray(v, dtype="d"), (len(pts),)).copy()
    return out


@functools.lru_cache(maxsize=None)
def split_points(op):
    """-> (indices of the accuracy points, indices of the points of POINTS that go to the conventions test): a point is an accuracy
    point when the truth's value and every derivative round to finite doubles and the oracle's are finite too."""
    tr, orc = truths(op), oracle_outputs(op, POINTS[op])
    acc, conv = [], []
    for i, (t, g, _) in enumerate(tr):
        fin = all(math.isfinite(_to_double(w)) for w in [t] + list(g)) and all(math.isfinite(orc[o][i]) for o in orc)
        (acc if fin else conv).append(i)
    return tuple(acc), tuple(conv)


def errors(op, outputs, idx=None):
    """{output: [e per accuracy point]} of `outputs` ({output: array over ALL points of POINTS[op]}) against the truths"""
    tr, pts = truths(op), POINTS[op]
    acc = split_points(op)[0] if idx is None else idx
    out = {}
    for j, o in enumerate(OUTPUTS[: 1 + pts.shape[1]]):
        if o not in outputs:
            continue
        es = []
        for i in acc:
            t, g, h = tr[i]
            es.append(measure(outputs[o][i], t, g, pts[i]) if j == 0 else measure(outputs[o][i], g[j - 1], h[j - 1], pts[i]))
        out[o] = es
    return out


# ---- regimes: (name, predicate on the point, the code branch it serves) ---------------------------------------------------------
def _iv(lo, hi, key=lambda p: p[0]):
    return lambda p: lo <= key(p) < hi


INF = math.inf
_GAMMA_REG = [("reflected_negative", _iv(-INF, 0.0), "x < 0.5: reflection, pi / tan(pi x), sin(pi x)"),
              ("reflected_small", _iv(0.0, 0.5), "x < 0.5: reflection with 1 - x in (0.5, 1]"),
              ("recurrence", _iv(0.5, 10.0), "0.5 <= x < 10: recurrence up to 10, then the series"),
              ("asymptotic", _iv(10.0, INF), "x >= 10: the asymptotic series alone")]
_ERF_REG = [("below_-1", _iv(-INF, -1.0), "library call, negative tail"), ("core", _iv(-1.0, 1.0), "library call, |x| < 1"),
            ("1_to_10", _iv(1.0, 10.0), "library call; d erfcx = 2 x v - 2/sqrt(pi) starts to cancel"),
            ("10_to_26.5", _iv(10.0, 26.5), "library call; d erfcx cancels"),
            ("26.5_to_1e3", _iv(26.5, 1e3), "erfc is denormal, then 0 (SciPy's flushes to 0 from 26.6 on); d erfcx cancels"),
            ("1e3_up", _iv(1e3, INF), "erfcx ~ 1/(x sqrt pi); d erfcx cancels completely")]
_SIG_REG = [("below_-37", _iv(-INF, -37.0), "softplus: exp(x)"), ("-37_to_0", _iv(-37.0, 0.0), "softplus: log1p(exp(x)); sigmoid: e / (1 + e)"),
            ("0_to_18", _iv(0.0, 18.0), "softplus: log1p(exp(x)); sigmoid: 1 / (1 + e); s (1 - s) cancels towards 18"),
            ("18_to_33.3", _iv(18.0, 33.3), "softplus: x + exp(-x); s (1 - s) cancels"), ("33.3_up", _iv(33.3, INF), "softplus: x; s (1 - s) cancels completely")]
_D = lambda p: p[0] - p[1]      # noqa: E731
REGIMES = {
    "digamma": _GAMMA_REG, "gammaln": _GAMMA_REG, "erf": _ERF_REG, "erfc": _ERF_REG, "erfcx": _ERF_REG,
    "log1mexp": [("near_0", _iv(-LOG2, INF), "x > -log 2: log(-expm1(x))"), ("far", _iv(-INF, -LOG2), "x <= -log 2: log1p(-exp(x))")],
    "softplus": _SIG_REG, "sigmoid": _SIG_REG,
    "logaddexp": [("x_below_y", _iv(-INF, 0.0, _D), "t <= 0: y + log1p(exp(t))"), ("equal", lambda p: p[0] == p[1], "x == y: x + log 2"),
                  ("x_above_y", lambda p: p[0] > p[1], "t > 0: x + log1p(exp(-t))")],
    "expm1": [("below_-1", _iv(-INF, -1.0), "d = v + 1 cancels"), ("core", _iv(-1.0, 1.0), "library call"), ("above_1", _iv(1.0, INF), "library call")],
    "exp": [("all", _iv(-INF, INF), "library call")],
    "log1p": [("near_-1", _iv(-1.0, -0.5), "library call"), ("core", _iv(-0.5, 1.0), "library call"), ("above_1", _iv(1.0, INF), "library call")],
    "tanh": [("core", _iv(0.0, 1.0, lambda p: abs(p[0])), "library call"), ("1_to_19", _iv(1.0, 19.1, lambda p: abs(p[0])), "d = 1 - v v cancels"),
             ("saturated", _iv(19.1, INF, lambda p: abs(p[0])), "v = +-1: d = 1 - v v cancels completely")],
    "pow": [("x_to_0", _iv(0.0, 1e-7), "library pow, x -> 0+, y <= 1"), ("x_next_to_1", lambda p: 0.5 < p[0] < 1.5 and abs(p[1]) >= 1e15, "library pow, x = 1 +- ulp, huge y"),
            ("general", lambda p: True, "library pow")],
    "log": [("near_1", _iv(0.25, 4.0), "library call"), ("far", lambda p: True, "library call, denormal and huge arguments")],
    "sqrt": [("denormal", _iv(0.0, 2.2250738585072014e-308), "sqrt instruction sequence, denormal input"), ("normal", lambda p: True, "sqrt instruction sequence")],
    "reciprocal": [("all", lambda p: True, "1 / x; d = -v v")],
    "div": [("all", lambda p: True, "x / y; d = g / y, -g v / y")],
    "maximum": [("all", lambda p: True, "select")], "minimum": [("all", lambda p: True, "select")],
    "clip": [("all", lambda p: True, "select")], "switch": [("all", lambda p: True, "select")],
}


def regime_of(op, pt):
    for name, pred, _ in REGIMES[op]:
        if pred(pt):
            return name
    raise AssertionError(f"{op}: point {pt} belongs to no regime")


def regime_errors(op, outputs):
    """{"op/regime/output": max e over the regime's accuracy points}; every accuracy point lands in exactly one regime"""
    acc = split_points(op)[0]
    es = errors(op, outputs)
    out = {}
    for o, col in es.items():
        for i, e in zip(acc, col):
            k = f"{op}/{regime_of(op, POINTS[op][i])}/{o}"
            out[k] = max(out.get(k, 0.0), e)
    return out


def bound(key):
    return FACTOR * max(1.0, E_O[key])


# A derivative the reference writes on the op's own VALUE v in a form that cancels: d erfcx = 2 x v - 2 / sqrt(pi), where one ulp of v
# is 2 x ulp(v) ~ 2e-16 in the result however small the true derivative -1 / (x x sqrt(pi)) is.  What the oracle shows of that loss
# depends on which way SciPy's v happens to round: 2 x erfcx(x) is exactly 2 / sqrt(pi) at 1e150 with SciPy's value (error 4.5e15) and
# one ulp off with the device library's (error 2.5e299), both values within half an ulp of erfcx.  So the reference's error in erfcx's
# derivative is taken over the reference's formula at the correctly rounded v and its two neighbours -- the accuracy any libm
# grants -- next to the oracle's own result.  (s (1 - s), 1 - t t and expm1(x) + 1 cancel as well; there the device's value and
# SciPy's round alike and the oracle's own error is the bound.)
CANCELLING = {"erfcx": lambda x, v: 2.0 * x * v - 2.0 / math.sqrt(math.pi)}


def reference_regime_errors(op):
    """E_O: the oracle's error per regime; for the ops of CANCELLING the derivative's error is the worst of the oracle's and of the
    reference's formula at v = RN(T) and its neighbours"""
    pts = POINTS[op]
    out = regime_errors(op, oracle_outputs(op, pts))
    if op in CANCELLING:
        v0 = np.asarray([_to_double(t[0]) for t in truths(op)])
        for v in (np.nextafter(v0, -np.inf), v0, np.nextafter(v0, np.inf)):
            with np.errstate(all="ignore"):
                for k, e in regime_errors(op, {"dx": CANCELLING[op](pts[:, 0], v)}).items():
                    out[k] = max(out[k], e)
    return out


# the oracle's error per regime (tests/test_scalar_edges.py asserts: computed <= tabulated <= 1.5 computed + 1).  Entries far above
# 1 are regimes where the REFERENCE's formula cancels (the branch notes above say which); the device uses the same formula there.
E_O = {
    # E_O_TABLE_BEGIN
    "digamma/reflected_small/v": 0.38, "digamma/recurrence/v": 0.43, "digamma/asymptotic/v": 1.1,
    "digamma/reflected_negative/v": 4.1, "digamma/reflected_small/dx": 0.74, "digamma/recurrence/dx": 0.66,
    "digamma/asymptotic/dx": 0.84, "digamma/reflected_negative/dx": 0.99, "gammaln/reflected_small/v": 0.53,
    "gammaln/recurrence/v": 7, "gammaln/asymptotic/v": 0.73, "gammaln/reflected_negative/v": 1.9,
    "gammaln/reflected_small/dx": 0.38, "gammaln/recurrence/dx": 0.43, "gammaln/asymptotic/dx": 1.1,
    "gammaln/reflected_negative/dx": 4.1, "erf/below_-1/v": 0.22, "erf/core/v": 0.43, "erf/1_to_10/v": 0.43,
    "erf/10_to_26.5/v": 0.01, "erf/26.5_to_1e3/v": 0.01, "erf/1e3_up/v": 0, "erf/below_-1/dx": 0.24, "erf/core/dx": 0.57,
    "erf/1_to_10/dx": 0.21, "erf/10_to_26.5/dx": 0.24, "erf/26.5_to_1e3/dx": 0.24, "erf/1e3_up/dx": 0, "erfc/below_-1/v": 0.14,
    "erfc/core/v": 0.55, "erfc/1_to_10/v": 0.26, "erfc/10_to_26.5/v": 0.24, "erfc/26.5_to_1e3/v": 1.1e+05, "erfc/1e3_up/v": 0,
    "erfc/below_-1/dx": 0.24, "erfc/core/dx": 0.57, "erfc/1_to_10/dx": 0.21, "erfc/10_to_26.5/dx": 0.24,
    "erfc/26.5_to_1e3/dx": 0.24, "erfc/1e3_up/dx": 0, "erfcx/below_-1/v": 0.24, "erfcx/core/v": 0.98, "erfcx/1_to_10/v": 0.95,
    "erfcx/10_to_26.5/v": 0.62, "erfcx/26.5_to_1e3/v": 0.28, "erfcx/1e3_up/v": 0.4, "erfcx/below_-1/dx": 0.24,
    "erfcx/core/dx": 1.7, "erfcx/1_to_10/dx": 58, "erfcx/10_to_26.5/dx": 750, "erfcx/26.5_to_1e3/dx": 1.1e+06,
    "erfcx/1e3_up/dx": 7.9e+299, "log1mexp/near_0/v": 0.5, "log1mexp/far/v": 0.43, "log1mexp/near_0/dx": 0.44,
    "log1mexp/far/dx": 0.58, "softplus/33.3_up/v": 0.25, "softplus/below_-37/v": 0.43, "softplus/-37_to_0/v": 0.27,
    "softplus/0_to_18/v": 0.26, "softplus/18_to_33.3/v": 0.25, "softplus/33.3_up/dx": 0.92, "softplus/below_-37/dx": 0.58,
    "softplus/-37_to_0/dx": 0.5, "softplus/0_to_18/dx": 1.2, "softplus/18_to_33.3/dx": 1.1, "sigmoid/33.3_up/v": 0.92,
    "sigmoid/below_-37/v": 0.58, "sigmoid/-37_to_0/v": 0.5, "sigmoid/0_to_18/v": 1.2, "sigmoid/18_to_33.3/v": 1.1,
    "sigmoid/33.3_up/dx": 7e+13, "sigmoid/below_-37/dx": 0.58, "sigmoid/-37_to_0/dx": 0.31, "sigmoid/0_to_18/dx": 1.4e+06,
    "sigmoid/18_to_33.3/dx": 4.1e+12, "logaddexp/x_above_y/v": 0.25, "logaddexp/x_below_y/v": 0.66, "logaddexp/equal/v": 0.21,
    "logaddexp/x_above_y/dx": 1.2, "logaddexp/x_below_y/dx": 0.58, "logaddexp/equal/dx": 0, "logaddexp/x_above_y/dy": 0.58,
    "logaddexp/x_below_y/dy": 1.2, "logaddexp/equal/dy": 0, "expm1/core/v": 0.21, "expm1/above_1/v": 0.1,
    "expm1/below_-1/v": 0.09, "expm1/core/dx": 0.5, "expm1/above_1/dx": 0.3, "expm1/below_-1/dx": 1.4e+14,
    "log1p/near_-1/v": 0.07, "log1p/core/v": 0.2, "log1p/above_1/v": 0.3, "log1p/near_-1/dx": 0.01, "log1p/core/dx": 0.65,
    "log1p/above_1/dx": 0.5, "tanh/core/v": 0.38, "tanh/1_to_19/v": 0.57, "tanh/saturated/v": 0.01, "tanh/core/dx": 0.43,
    "tanh/1_to_19/dx": 1.4e+14, "tanh/saturated/dx": 7e+13, "pow/x_to_0/v": 0.37, "pow/x_next_to_1/v": 0.01,
    "pow/general/v": 0.2, "pow/x_to_0/dx": 77, "pow/x_next_to_1/dx": 0.01, "pow/general/dx": 0.13, "pow/x_to_0/dy": 0.74,
    "pow/x_next_to_1/dy": 0.01, "pow/general/dy": 0.16, "log/near_1/v": 0.11, "log/far/v": 0.21, "log/near_1/dx": 0.34,
    "log/far/dx": 0.25, "sqrt/denormal/v": 0.01, "sqrt/normal/v": 0.34, "sqrt/denormal/dx": 0.34, "sqrt/normal/dx": 0.6,
    "reciprocal/all/v": 0.34, "reciprocal/all/dx": 0.32, "exp/all/v": 0.43, "exp/all/dx": 0.43, "div/all/v": 0.34,
    "div/all/dx": 0.26, "div/all/dy": 0.2, "maximum/all/v": 0, "maximum/all/dx": 0, "maximum/all/dy": 0, "minimum/all/v": 0,
    "minimum/all/dx": 0, "minimum/all/dy": 0, "clip/all/v": 0, "clip/all/dx": 0, "clip/all/dy": 0, "clip/all/dz": 0,
    "switch/all/v": 0, "switch/all/dx": 0, "switch/all/dy": 0, "switch/all/dz": 0,
    # E_O_TABLE_END
}


# ---- the isolating models -------------------------------------------------------------------------------------------------------
def _apply(m, op, xs):
    M = m.math
    if op in ("clip", "switch"):
        return getattr(M, op)(*xs)
    if len(xs) == 2:
        return xs[0] / xs[1] if op == "div" else getattr(M, op)(*xs)
    return getattr(M, op)(xs[0])


def permutation(n):
    return np.random.default_rng(1000 + n).permutation(n)


def build_model(groups, gather=False):
    """groups: [(op, points [n, arity])] -> (spec, q, layout).  One Potential `s * op(x[, y, z])` per group over Flat vectors of its
    own; with `gather` the operands are read through `x[idx]`, idx a fixed permutation.  q holds the points (s = 1).
    layout[i] = {"s": slice, "x": index array, ...}: where the group's outputs sit in the gradient, in point order."""
    m = ModelBuilder()
    q, layout, off = [], [], 0
    for gi, (op, pts) in enumerate(groups):
        n, ar = pts.shape
        perm = permutation(n)
        where, xs = {}, []
        for k in range(ar):
            v = m.Flat(f"{op}{gi}_{'xyz'[k]}", shape=(n,))
            if gather:
                xs.append(v[perm])
                col = np.empty(n)
                col[perm] = pts[:, k]
                where["d" + "xyz"[k]] = off + perm
            else:
                xs.append(v)
                col = pts[:, k]
                where["d" + "xyz"[k]] = off + np.arange(n)
            q.append(col)
            off += n
        s = m.Flat(f"{op}{gi}_s", shape=(n,))
        q.append(np.ones(n))
        where["v"] = off + np.arange(n)
        off += n
        m.Potential(f"{op}{gi}", s * _apply(m, op, xs))
        layout.append(where)
    return m.build(), np.concatenate(q), layout


def read_outputs(layout_entry, grad):
    return {o: np.asarray(grad)[ix] for o, ix in layout_entry.items()}


HUGE = 1e150


def accuracy_groups():
    """[(model name, [(op, indices into POINTS[op])])]: the accuracy points, a few ops per model; points with an output beyond 1e150
    in a model of their own (its log-density must stay finite too)."""
    ops = list(POINTS)
    plain, huge = {}, []
    for op in ops:
        acc = split_points(op)[0]
        tr = truths(op)
        big = [i for i in acc if any(abs(_to_double(w)) > HUGE for w in [tr[i][0]] + list(tr[i][1]))]
        plain[op] = [i for i in acc if i not in big]
        if big:
            huge.append((op, big))
    chunks = [ops[i:i + 3] for i in range(0, len(ops), 3)]
    return [("_".join(c), [(op, plain[op]) for op in c if plain[op]]) for c in chunks] + [("huge", huge)]


def klass(a):
    return "nan" if a != a else ("+inf" if a == math.inf else ("-inf" if a == -math.inf else "finite"))


def convention_groups():
    """[(op, points)]: CONVENTION_POINTS and the points of POINTS that `split_points` kept out of the accuracy models"""
    out = []
    for op in POINTS:
        conv = list(split_points(op)[1])
        pts = [POINTS[op][conv]] if conv else []
        if op in CONVENTION_POINTS:
            pts.append(CONVENTION_POINTS[op])
        if pts:
            out.append((op, np.concatenate(pts)))
    return out


def group_points(groups):
    """[(op, indices into POINTS[op]) or (op, points)] -> [(op, points)]"""
    return [(op, sel if isinstance(sel, np.ndarray) else POINTS[op][list(sel)]) for op, sel in groups]


def scatter(op, idx, outputs, into=None):
    """outputs of a model group (point order `idx`) into arrays over ALL points of POINTS[op] (NaN where not evaluated)"""
    into = {} if into is None else into
    for o, col in outputs.items():
        full = into.setdefault(o, np.full(len(POINTS[op]), np.nan))
        full[list(idx)] = col
    return into


# ---- densities: observed factors whose parameters are Flat vectors ---------------------------------------------------------------
# The element-wise log-density comes back through `DeviceValueGradFunction.log_likelihood` (k_ll_factor), the partials w.r.t. the
# parameters through the gradient: every Flat vector occurs in ONE factor, element-aligned, so grad[param_i] is the partial of
# element i.  A case is one factor (its constants choose the branch of csrc/model_dev.h `dist_eval_body` it runs) and one regime.
def _log_ndtr_diff(za, zb):
    """log(Phi(zb) - Phi(za)), None: unbounded; each in the form that does not cancel"""
    r2 = mp.sqrt(2)
    if za is None:
        return mp.log(mp.erfc(-zb / r2) / 2)
    if zb is None:
        return mp.log(mp.erfc(za / r2) / 2)
    if za > 0:
        return mp.log((mp.erfc(za / r2) - mp.erfc(zb / r2)) / 2)
    if zb < 0:
        return mp.log((mp.erfc(-zb / r2) - mp.erfc(-za / r2)) / 2)
    return mp.log((mp.erf(zb / r2) - mp.erf(za / r2)) / 2)


def _lg(x):
    return gamma_family(x)[0]


def _mp_logp(kind, c, y, p):
    """log-density in mpf: kind, constants c, value y, parameters p (the Flat vectors' elements, in the builder's order)"""
    if kind == "TruncatedNormal":
        mu, sg = p
        lo, hi = c["lower"], c["upper"]
        za = None if lo is None else (mp.mpf(lo) - mu) / sg
        zb = None if hi is None else (mp.mpf(hi) - mu) / sg
        z = (y - mu) / sg
        return -z * z / 2 - mp.log(2 * mp.pi) / 2 - mp.log(sg) - _log_ndtr_diff(za, zb)
    if kind == "StudentT":
        mu, sg = p
        nu = mp.mpf(c["nu"])
        z = (y - mu) / sg
        return _lg((nu + 1) / 2) - _lg(nu / 2) - mp.log(nu * mp.pi) / 2 - mp.log(sg) - (nu + 1) / 2 * mp.log1p(z * z / nu)
    if kind == "Cauchy":
        al, be = p
        z = (y - al) / be
        return -mp.log(mp.pi) - mp.log(be) - mp.log1p(z * z)
    if kind == "Gamma":
        al, (be,) = mp.mpf(c["alpha"]), p
        return al * mp.log(be) - _lg(al) + (al - 1) * mp.log(y) - be * y
    if kind == "InverseGamma":
        al, (be,) = mp.mpf(c["alpha"]), p
        return al * mp.log(be) - _lg(al) - (al + 1) * mp.log(y) - be / y
    if kind == "Beta":
        al, be = mp.mpf(c["alpha"]), mp.mpf(c["beta"])
        return (al - 1) * mp.log(y) + (be - 1) * mp.log1p(-y) - (_lg(al) + _lg(be) - _lg(al + be))
    if kind == "Binomial":          # y in {0, n}: the binomial coefficient is 1
        n, (pp,) = mp.mpf(c["n"]), p
        return y * mp.log(pp) + (n - y) * mp.log1p(-pp)
    if kind == "Bernoulli":
        return mp.log(p[0]) if y != 0 else mp.log1p(-p[0])
    if kind == "Poisson":
        return y * mp.log(p[0]) - _lg(y + 1) - p[0]
    if kind == "BernoulliLogit":
        return -mp.log1p(mp.exp(-p[0])) if y != 0 else -mp.log1p(mp.exp(p[0]))
    raise KeyError(kind)


def _grid(ys, *cols):
    """cartesian product -> (y, [param columns])"""
    import itertools
    rows = list(itertools.product(ys, *cols))
    a = np.asarray(rows, dtype="d")
    return a[:, 0], [a[:, k] for k in range(1, a.shape[1])]


def _tn_case(name, za, zb, note):
    mu, sg = 0.5, 2.0
    lo = None if za is None else mu + sg * za
    hi = None if zb is None else mu + sg * zb
    if lo is not None and hi is not None:
        ys = [lo, (lo + hi) / 2, hi]
    elif lo is not None:
        ys = [lo, lo + sg, lo + 10 * sg]
    else:
        ys = [hi, hi - sg, hi - 10 * sg]
    y = np.asarray(ys)
    return dict(name=name, kind="TruncatedNormal", const=dict(lower=lo, upper=hi), y=y, params=[np.full(3, mu), np.full(3, sg)], args=(1, 2), note=note)


def _density_cases():
    cases = []
    for za, zb, note in ((-40.0, -30.0, "log_diff_normal_cdf: x < 0, erfcx(-x) - exp(x x - y y) erfcx(-y)"), (30.0, 40.0, "log_diff_normal_cdf: y > 0, erfcx(y) - exp(y y - x x) erfcx(x)"),
                         (-1.0, 1.0, "log_diff_normal_cdf: log(erf(x) - erf(y))"), (0.999, 1.001, "log_diff_normal_cdf: y > 0, narrow interval")):
        cases.append(_tn_case(f"tn[{za:g},{zb:g}]", za, zb, note))
    for za in (-40.0, 0.999, 1.001, 30.0):
        cases.append(_tn_case(f"tn[{za:g},inf)", za, None, "normal_lccdf: " + ("erfcx tail" if za > 1 else "log1p(-erfc / 2)")))
        cases.append(_tn_case(f"tn(-inf,{-za:g}]", None, -za, "normal_lcdf: " + ("erfcx tail" if za > 1 else "log1p(-erfc / 2)")))
    z = np.asarray([1e-8, 1.0, 1e8, 1e150] * 2)
    mu, sg = np.repeat([0.5, 0.0], 4), np.repeat([2.0, 1.0], 4)
    cases.append(dict(name="studentt", kind="StudentT", const=dict(nu=4.0), y=mu + sg * z, params=[mu, sg], args=(2, 3), note="log1p(z z / nu), w = (nu + 1) z / (nu + z z) up to z = 1e150"))
    cases.append(dict(name="cauchy", kind="Cauchy", const={}, y=mu + sg * z, params=[mu.copy(), sg.copy()], args=(1, 2), note="log1p(z z), w = 2 z / (1 + z z) up to z = 1e150"))
    for al in (0.5, 1.0, float(np.nextafter(1.0, 2.0)), 50.0):
        tag = "1+ulp" if 1.0 < al < 1.5 else f"{al:g}"
        y, (be,) = _grid([1e-300, 1e-8, 1e8], [1.0, 2.5])
        cases.append(dict(name=f"gamma[{tag}]", kind="Gamma", const=dict(alpha=al), y=y, params=[be], args=(2,), note="logpow(value, alpha - 1)" + (": the m == 0 case" if al == 1.0 else "")))
        y, (be,) = _grid([1e-8, 1e8], [1.0, 2.5])
        cases.append(dict(name=f"invgamma[{tag}]", kind="InverseGamma", const=dict(alpha=al), y=y, params=[be], args=(2,), note="logpow(value, -alpha - 1)"))
        cases.append(dict(name=f"invgamma[{tag}]@1e-300", kind="InverseGamma", const=dict(alpha=al), y=np.full(2, 1e-300), params=[np.asarray([1.0, 2.5])], args=(2,),
                          note="-beta / value = -1e300", huge=True))
    for al, be in ((0.5, 0.5), (2.0, 3.0), (1.0, 1.0)):
        cases.append(dict(name=f"beta[{al:g},{be:g}]", kind="Beta", const=dict(alpha=al, beta=be), y=np.asarray([1e-300, 1e-16, 1.0 - 2.0 ** -53]), params=[], args=(),
                          note="(alpha - 1) log v + (beta - 1) log1p(-v)" + (": both skipped" if al == 1.0 else "")))
    y, (p,) = _grid([0.0, 10.0], [1e-300, 1.0 - 2.0 ** -53])
    cases.append(dict(name="binomial", kind="Binomial", const=dict(n=10.0), y=y, params=[p], args=(2,), note="logpow(p, y) + logpow(1 - p, n - y) at y in {0, n}"))
    y, (p,) = _grid([0.0, 1.0], [1e-300, 1.0 - 2.0 ** -53])
    cases.append(dict(name="bernoulli", kind="Bernoulli", const={}, y=y, params=[p], args=(1,), note="log(p) | log1p(-p)"))
    y, (m_,) = _grid([0.0, 3.0], [1e-300, 1e8])
    cases.append(dict(name="poisson", kind="Poisson", const={}, y=y, params=[m_], args=(1,), note="logpow(mu, y) - mu"))
    y, (eta,) = _grid([0.0, 1.0], [800.0, -800.0])
    cases.append(dict(name="bernoulli_logit", kind="BernoulliLogit", const={}, y=y, params=[eta], args=(1,), note="-softplus(-+eta), y - sigmoid(eta)"))
    return cases


DENSITY_CASES = _density_cases()
for _i, _c in enumerate(DENSITY_CASES):
    _c["ci"] = _i


def density_models():
    """[(model name, [cases])]: the cases whose log-density is near 1e300 in a model of their own"""
    return [("densities", [c for c in DENSITY_CASES if not c.get("huge")]), ("densities_huge", [c for c in DENSITY_CASES if c.get("huge")])]


def build_density_model(cases):
    """-> (spec, q, layout): layout[i] = index arrays of case i's parameter vectors in q / the gradient"""
    m = ModelBuilder()
    q, layout, off = [], [], 0
    for ci, c in enumerate(cases):
        n, exprs, where = len(c["y"]), [], []
        for k, col in enumerate(c["params"]):
            exprs.append(m.Flat(f"c{ci}_p{k}", shape=(n,)))
            q.append(np.asarray(col, dtype="d"))
            where.append(off + np.arange(n))
            off += n
        k_, kw = c["kind"], c["const"]
        if k_ == "TruncatedNormal":
            m.TruncatedNormal(c["name"], exprs[0], exprs[1], lower=kw["lower"], upper=kw["upper"], observed=c["y"])
        elif k_ == "StudentT":
            m.StudentT(c["name"], kw["nu"], exprs[0], exprs[1], observed=c["y"])
        elif k_ == "Cauchy":
            m.Cauchy(c["name"], exprs[0], exprs[1], observed=c["y"])
        elif k_ in ("Gamma", "InverseGamma"):
            getattr(m, k_)(c["name"], kw["alpha"], exprs[0], observed=c["y"])
        elif k_ == "Beta":
            m.Beta(c["name"], kw["alpha"], kw["beta"], observed=c["y"])
        elif k_ == "Binomial":
            m.Binomial(c["name"], kw["n"], exprs[0], observed=c["y"])
        else:
            getattr(m, k_)(c["name"], exprs[0], observed=c["y"])
        layout.append(where)
    if not q:
        raise ValueError("a density model needs at least one parameter vector")
    return m.build(), np.concatenate(q), layout


def oracle_density_outputs(spec, q, cases):
    """[{"lp": ..., "d1": ..., ...}] per case from oracle/ref_models.py `_forward` + `_dist` (dK: partial w.r.t. the K-th Flat parameter)"""
    out = []
    by_name = {f.name: f for f in spec.factors}
    with np.errstate(all="ignore"):
        for c in cases:
            f = by_name[c["name"]]
            args = rm._forward(spec, f, np.asarray(q, dtype="d"))[0]
            lp, parts = rm._dist(f.dist, f.konst, args)
            n = len(c["y"])
            o = {"lp": np.broadcast_to(np.asarray(lp, dtype="d"), (n,)).copy()}
            for k, a in enumerate(c["args"]):
                o[f"d{k + 1}"] = np.broadcast_to(np.asarray(parts[a], dtype="d"), (n,)).copy()
            out.append(o)
    return out


def _density_truth_at(c, i, prec, second=False):
    """(lp, [partials]) of element i of case c by central differences of the mpf log-density with a relative step of 2^-(2 prec / 5):
    truncation and rounding both below 2^-(3 prec / 5) of (|lp| + 1) / |parameter|; a partial below 2^-(prec / 2 + 100) of that scale
    is an exact zero of the truth ((z z - 1) / sigma at z = 1) -- with a scale near 1 it is below the smallest double anyway.
    `second`: the second partials (the measure's denominators only)"""
    with mp.workprec(prec):
        y = mp.mpf(float(c["y"][i]))
        p0 = [mp.mpf(float(col[i])) for col in c["params"]]
        hs = [(abs(a) if a != 0 else mp.mpf(1)) * mp.ldexp(1, -(2 * prec // 5)) for a in p0]

        def f(p):
            return _mp_logp(c["kind"], c["const"], y, p)

        def d1(k, p):
            up, dn = list(p), list(p)
            up[k] += hs[k]
            dn[k] -= hs[k]
            return (f(up) - f(dn)) / (2 * hs[k])

        if not second:
            t = f(p0)
            g = [d1(k, p0) for k in range(len(p0))]
            tiny = [(abs(t) + 1) / (abs(a) if a != 0 else mp.mpf(1)) * mp.ldexp(1, -(prec // 2 + 100)) for a in p0]
            return t, [mp.mpf(0) if abs(d) < lim else d for d, lim in zip(g, tiny)]
        hess = []
        for k in range(len(p0)):
            row = []
            for j in range(len(p0)):
                up, dn = list(p0), list(p0)
                up[j] += hs[j]
                dn[j] -= hs[j]
                row.append((d1(k, up) - d1(k, dn)) / (2 * hs[j]))
            hess.append(row)
        return hess


@functools.lru_cache(maxsize=None)
def density_truths(ci):
    c, out = DENSITY_CASES[ci], []
    for i in range(len(c["y"])):
        a, b = _density_truth_at(c, i, PREC), _density_truth_at(c, i, 2 * PREC)
        fa, fb = [_to_double(w) for w in [a[0]] + a[1]], [_to_double(w) for w in [b[0]] + b[1]]
        assert fa == fb and all(math.isfinite(w) for w in fa), (c["name"], i, fa, fb)
        out.append((a[0], a[1], _density_truth_at(c, i, 600, second=True)))
    return out


def density_errors(ci, outputs):
    """{"density/case/output": max e over the case's elements}: the measure of the module docstring with the Flat parameters as the
    inputs (the observed value and the constants are exact data)"""
    c, tr, out = DENSITY_CASES[ci], density_truths(ci), {}
    for i, (t, g, h) in enumerate(tr):
        pt = [float(col[i]) for col in c["params"]]
        for o, col in outputs.items():
            e = measure(col[i], t, g, pt) if o == "lp" else measure(col[i], g[int(o[1:]) - 1], h[int(o[1:]) - 1], pt)
            k = f"density/{c['name']}/{o}"
            out[k] = max(out.get(k, 0.0), e)
    return out


def reference_density_errors():
    out = {}
    for _, cases in density_models():
        spec, q, _ = build_density_model(cases)
        for c, o in zip(cases, oracle_density_outputs(spec, q, cases)):
            out.update(density_errors(c["ci"], o))
    return out


def density_bound(key):
    return FACTOR * max(1.0, E_O_DENSITY[key])


# the oracle's error per density case (asserted like E_O).  The large entries are the reference's own cancellations: the partials of
# the truncated normal's normaliser at bounds tens of sigmas out, (z z - 1) / sigma at z = 1, ...
E_O_DENSITY = {
    # E_O_DENSITY_BEGIN
    "density/tn[-40,-30]/lp": 93, "density/tn[-40,-30]/d1": 3.5e+05, "density/tn[-40,-30]/d2": 1.1e+05,
    "density/tn[30,40]/lp": 93, "density/tn[30,40]/d1": 3.5e+05, "density/tn[30,40]/d2": 1.1e+05, "density/tn[-1,1]/lp": 0.46,
    "density/tn[-1,1]/d1": 0, "density/tn[-1,1]/d2": 0.81, "density/tn[0.999,1.001]/lp": 190,
    "density/tn[0.999,1.001]/d1": 8e+08, "density/tn[0.999,1.001]/d2": 7.4e+08, "density/tn[-40,inf)/lp": 0.08,
    "density/tn[-40,inf)/d1": 0, "density/tn[-40,inf)/d2": 0, "density/tn(-inf,40]/lp": 0.08, "density/tn(-inf,40]/d1": 0,
    "density/tn(-inf,40]/d2": 0, "density/tn[0.999,inf)/lp": 0.89, "density/tn[0.999,inf)/d1": 2.6,
    "density/tn[0.999,inf)/d2": 1.2, "density/tn(-inf,-0.999]/lp": 0.36, "density/tn(-inf,-0.999]/d1": 0.16,
    "density/tn(-inf,-0.999]/d2": 0.31, "density/tn[1.001,inf)/lp": 0.87, "density/tn[1.001,inf)/d1": 2.4,
    "density/tn[1.001,inf)/d2": 0.43, "density/tn(-inf,-1.001]/lp": 0.87, "density/tn(-inf,-1.001]/d1": 2.4,
    "density/tn(-inf,-1.001]/d2": 0.43, "density/tn[30,inf)/lp": 35, "density/tn[30,inf)/d1": 1.5e+05,
    "density/tn[30,inf)/d2": 4.5e+04, "density/tn(-inf,-30]/lp": 35, "density/tn(-inf,-30]/d1": 1.5e+05,
    "density/tn(-inf,-30]/d2": 4.5e+04, "density/studentt/lp": 2.8, "density/studentt/d1": 0.82, "density/studentt/d2": 0.5,
    "density/cauchy/lp": 0.81, "density/cauchy/d1": 0.91, "density/cauchy/d2": 1, "density/gamma[0.5]/lp": 0.46,
    "density/gamma[0.5]/d1": 0.26, "density/invgamma[0.5]/lp": 1.3, "density/invgamma[0.5]/d1": 0.26,
    "density/gamma[1]/lp": 0.29, "density/gamma[1]/d1": 0.4, "density/invgamma[1]/lp": 0.59, "density/invgamma[1]/d1": 0.26,
    "density/gamma[1+ulp]/lp": 1, "density/gamma[1+ulp]/d1": 0.4, "density/invgamma[1+ulp]/lp": 0.38,
    "density/invgamma[1+ulp]/d1": 0.26, "density/gamma[50]/lp": 0.86, "density/gamma[50]/d1": 0.12,
    "density/invgamma[50]/lp": 0.44, "density/invgamma[50]/d1": 0.15, "density/beta[0.5,0.5]/lp": 0.47,
    "density/beta[2,3]/lp": 0.28, "density/beta[1,1]/lp": 0.01, "density/binomial/lp": 0.51, "density/binomial/d1": 0.24,
    "density/bernoulli/lp": 0.21, "density/bernoulli/d1": 0.34, "density/poisson/lp": 0.1, "density/poisson/d1": 0.36,
    "density/bernoulli_logit/lp": 0.01, "density/bernoulli_logit/d1": 0, "density/invgamma[0.5]@1e-300/lp": 0.2,
    "density/invgamma[0.5]@1e-300/d1": 0.48, "density/invgamma[1]@1e-300/lp": 0.2, "density/invgamma[1]@1e-300/d1": 0.48,
    "density/invgamma[1+ulp]@1e-300/lp": 0.2, "density/invgamma[1+ulp]@1e-300/d1": 0.48, "density/invgamma[50]@1e-300/lp": 0.2,
    "density/invgamma[50]@1e-300/d1": 0.48,
    # E_O_DENSITY_END
}


# ---- free variables: d logp / d value without a transform, and the log, log-odds and interval transforms -------------------------
# The gradient of a free vector whose parameters are constants is element-wise: d/dq of (logp(x(q)) + log|dx/dq|), transform_full
# and the density's d0 in csrc/model_dev.h.  Truth: central differences of that function in mpf.  Regimes: the branches of
# softplus_d / sigmoid_d along q (_SIG_REG) for the transforms, one per case without.
_Q = np.asarray([s * v for v in (1e-8, 1.0, 18.0, 33.3, 37.0, 40.0, 700.0) for s in (1.0, -1.0)])
_Z = np.asarray([1e-8, 1.0, 1e8, 1e150])


def _free_mp(name, q):
    ls, l1s = -mp.log1p(mp.exp(-q)), -mp.log1p(mp.exp(q))      # log s, log(1 - s), s = sigmoid(q)
    if name == "log/exponential":
        return -mp.exp(q) + q
    if name == "log/gamma[2.5,1.5]":
        return mp.mpf(2.5) * mp.log(mp.mpf(1.5)) - _lg(mp.mpf(2.5)) + mp.mpf(1.5) * q - mp.mpf(1.5) * mp.exp(q) + q
    if name == "logodds/beta[2,3]":
        return ls + 2 * l1s - (_lg(mp.mpf(2)) + _lg(mp.mpf(3)) - _lg(mp.mpf(5))) + ls + l1s
    if name == "interval/uniform[-1,3]":
        return ls + l1s
    if name == "interval/truncnormal[-1,3]":
        x = -1 + 4 / (1 + mp.exp(-q))
        return _mp_logp("TruncatedNormal", dict(lower=-1.0, upper=3.0), x, [mp.mpf(0.5), mp.mpf(2)]) + mp.log(4) + ls + l1s
    if name == "none/studentt":
        return _mp_logp("StudentT", dict(nu=4.0), q, [mp.mpf(0.5), mp.mpf(2)])
    if name == "none/cauchy":
        return _mp_logp("Cauchy", {}, q, [mp.mpf(0.5), mp.mpf(2)])
    if name == "none/gamma[0.5,2.5]":
        return _mp_logp("Gamma", dict(alpha=0.5), q, [mp.mpf(2.5)])
    if name == "none/gamma[50,2.5]":
        return _mp_logp("Gamma", dict(alpha=50.0), q, [mp.mpf(2.5)])
    if name == "none/invgamma[0.5,2.5]":
        return _mp_logp("InverseGamma", dict(alpha=0.5), q, [mp.mpf(2.5)])
    if name == "none/beta[0.5,0.5]":
        return _mp_logp("Beta", dict(alpha=0.5, beta=0.5), q, [])
    if name == "none/beta[2,3]":
        return _mp_logp("Beta", dict(alpha=2.0, beta=3.0), q, [])
    raise KeyError(name)


def _free_build(m, name, vname, n):
    if name == "log/exponential":
        return m.Exponential(vname, 1.0, shape=n)
    if name == "log/gamma[2.5,1.5]":
        return m.Gamma(vname, 2.5, 1.5, shape=n)
    if name == "logodds/beta[2,3]":
        return m.Beta(vname, 2.0, 3.0, shape=n)
    if name == "interval/uniform[-1,3]":
        return m.Uniform(vname, -1.0, 3.0, shape=n)
    if name == "interval/truncnormal[-1,3]":
        return m.TruncatedNormal(vname, 0.5, 2.0, lower=-1.0, upper=3.0, shape=n)
    if name == "none/studentt":
        return m.StudentT(vname, 4.0, 0.5, 2.0, shape=n)
    if name == "none/cauchy":
        return m.Cauchy(vname, 0.5, 2.0, shape=n)
    if name.startswith("none/gamma"):
        return m.Gamma(vname, 0.5 if "0.5," in name else 50.0, 2.5, shape=n, transform=None)
    if name == "none/invgamma[0.5,2.5]":
        return m.InverseGamma(vname, 0.5, 2.5, shape=n, transform=None)
    if name == "none/beta[0.5,0.5]":
        return m.Beta(vname, 0.5, 0.5, shape=n, transform=None)
    if name == "none/beta[2,3]":
        return m.Beta(vname, 2.0, 3.0, shape=n, transform=None)
    raise KeyError(name)


_V3, _B3 = np.asarray([1e-300, 1e-8, 1e8]), np.asarray([1e-300, 1e-16, 1.0 - 2.0 ** -53])
FREE_CASES = {
    "log/exponential": _Q, "log/gamma[2.5,1.5]": _Q, "logodds/beta[2,3]": _Q, "interval/uniform[-1,3]": _Q, "interval/truncnormal[-1,3]": _Q,
    "none/studentt": np.concatenate([0.5 + 2.0 * _Z, 0.5 - 2.0 * _Z]), "none/cauchy": np.concatenate([0.5 + 2.0 * _Z, 0.5 - 2.0 * _Z]),
    "none/gamma[0.5,2.5]": _V3, "none/gamma[50,2.5]": _V3, "none/invgamma[0.5,2.5]": _V3, "none/beta[0.5,0.5]": _B3, "none/beta[2,3]": _B3,
}


def build_free_model(sel):
    """sel: {case: indices into FREE_CASES[case]} -> (spec, q, {case: index array into q / the gradient})"""
    m = ModelBuilder()
    q, where, off = [], {}, 0
    for ci, (name, idx) in enumerate(sel.items()):
        if len(idx) == 0:
            continue
        _free_build(m, name, f"v{ci}", len(idx))
        q.append(FREE_CASES[name][list(idx)])
        where[name] = off + np.arange(len(idx))
        off += len(idx)
    return m.build(), np.concatenate(q), where


@functools.lru_cache(maxsize=None)
def free_truths(name):
    """[(f', f'') or None]: None where f or f' is not a finite double at the point"""
    out = []
    for qv in FREE_CASES[name]:
        res = []
        for prec in (PREC, 2 * PREC):
            with mp.workprec(prec):
                x = mp.mpf(float(qv))
                h = abs(x) * mp.ldexp(1, -(2 * prec // 5))
                f0, d = _free_mp(name, x), (_free_mp(name, x + h) - _free_mp(name, x - h)) / (2 * h)
                if abs(d) < (abs(f0) + 1) / abs(x) * mp.ldexp(1, -(prec // 2 + 100)):
                    d = mp.mpf(0)
                res.append((f0, d))
        assert _to_double(res[0][1]) == _to_double(res[1][1]), (name, qv)
        with mp.workprec(600):
            x = mp.mpf(float(qv))
            h = abs(x) * mp.ldexp(1, -120)
            d2 = (_free_mp(name, x + h) - 2 * _free_mp(name, x) + _free_mp(name, x - h)) / (h * h)
        fin = math.isfinite(_to_double(res[0][0])) and math.isfinite(_to_double(res[0][1]))
        out.append((res[0][1], d2, _to_double(res[0][0])) if fin else None)
    return out


def reference_free_errors():
    out = {}
    for name, sel in free_models()[:2]:
        lp, g = oracle_free_gradient(sel)
        assert math.isfinite(lp), (name, lp)
        free_errors(g, sel, out)
    return out


def oracle_free_gradient(sel):
    spec, q, where = build_free_model(sel)
    with np.errstate(all="ignore"):
        lp, grad = rm.evaluate(spec, q)
    return lp, {name: np.asarray(grad)[ix] for name, ix in where.items()}


@functools.lru_cache(maxsize=None)
def free_split():
    """({case: accuracy indices}, {case: convention indices}): accuracy where the truth is finite and the oracle, evaluated on the
    element ALONE, has a finite log-density and gradient"""
    acc, conv = {}, {}
    for name, pts in FREE_CASES.items():
        tr = free_truths(name)
        acc[name], conv[name] = [], []
        for i in range(len(pts)):
            lp, g = oracle_free_gradient({name: (i,)})
            ok = tr[i] is not None and math.isfinite(lp) and math.isfinite(g[name][0])
            (acc if ok else conv)[name].append(i)
    return {k: tuple(v) for k, v in acc.items()}, {k: tuple(v) for k, v in conv.items()}


def free_models():
    """[(model name, {case: indices})]: the accuracy points, those whose log-density is beyond 1e150 in a model of their own, and the
    convention points"""
    acc, conv = free_split()
    big = {k: tuple(i for i in v if abs(free_truths(k)[i][2]) > HUGE) for k, v in acc.items()}
    return [("free", {k: tuple(i for i in v if i not in big[k]) for k, v in acc.items()}), ("free_huge", {k: v for k, v in big.items() if v}),
            ("free_conventions", {k: v for k, v in conv.items() if v})]


def free_regime(name, qv):
    if name.startswith("none/"):
        return "all"
    return regime_of("sigmoid", (qv,))


def free_errors(grads, sel, out=None):
    """{"free/case/regime/dq": max e} of {case: gradient over the points `sel[case]`}"""
    out = {} if out is None else out
    for name, g in grads.items():
        tr = free_truths(name)
        for a, i in zip(g, sel[name]):
            qv = float(FREE_CASES[name][i])
            k = f"free/{name}/{free_regime(name, qv)}/dq"
            out[k] = max(out.get(k, 0.0), measure(a, tr[i][0], [tr[i][1]], (qv,)))
    return out


def free_bound(key):
    return FACTOR * max(1.0, E_O_FREE[key])


# the oracle's error (asserted like E_O).  The large entries: s (1 - s) and 1 - 2 s of the reference's transforms lose the digits of
# 1 - s beyond q = 18, and x(q) rounds onto the bound itself from q = 37 on.
E_O_FREE = {
    # E_O_FREE_BEGIN
    "free/log/exponential/0_to_18/dq": 3.4e+07, "free/log/exponential/-37_to_0/dq": 3.3e+06,
    "free/log/exponential/18_to_33.3/dq": 0.01, "free/log/exponential/33.3_up/dq": 0.02,
    "free/log/exponential/below_-37/dq": 0.02, "free/log/gamma[2.5,1.5]/0_to_18/dq": 2.5,
    "free/log/gamma[2.5,1.5]/-37_to_0/dq": 0.35, "free/log/gamma[2.5,1.5]/18_to_33.3/dq": 0.04,
    "free/log/gamma[2.5,1.5]/33.3_up/dq": 0.02, "free/log/gamma[2.5,1.5]/below_-37/dq": 0.02,
    "free/logodds/beta[2,3]/0_to_18/dq": 0.69, "free/logodds/beta[2,3]/-37_to_0/dq": 1.4,
    "free/logodds/beta[2,3]/18_to_33.3/dq": 0.86, "free/logodds/beta[2,3]/33.3_up/dq": 1.2,
    "free/logodds/beta[2,3]/below_-37/dq": 0.05, "free/interval/uniform[-1,3]/0_to_18/dq": 1.9e+07,
    "free/interval/uniform[-1,3]/-37_to_0/dq": 1.9e+07, "free/interval/uniform[-1,3]/18_to_33.3/dq": 0.24,
    "free/interval/uniform[-1,3]/33.3_up/dq": 1.9, "free/interval/uniform[-1,3]/below_-37/dq": 0.04,
    "free/interval/truncnormal[-1,3]/0_to_18/dq": 1.6, "free/interval/truncnormal[-1,3]/-37_to_0/dq": 3.6,
    "free/interval/truncnormal[-1,3]/18_to_33.3/dq": 0.24, "free/interval/truncnormal[-1,3]/33.3_up/dq": 0.23,
    "free/interval/truncnormal[-1,3]/below_-37/dq": 0.01, "free/none/studentt/all/dq": 0.45, "free/none/cauchy/all/dq": 0.39,
    "free/none/gamma[0.5,2.5]/all/dq": 0.23, "free/none/gamma[50,2.5]/all/dq": 0.3, "free/none/invgamma[0.5,2.5]/all/dq": 0.41,
    "free/none/beta[0.5,0.5]/all/dq": 0.38, "free/none/beta[2,3]/all/dq": 0.23,
    # E_O_FREE_END
}
