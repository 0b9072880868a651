"""The row passes' own logistic (pymc_amd/csrc/rows_kernel.h `logit_row` / `logit_row2`: a written-out exp, reciprocal and log1p) at
the edges of its domain: the point table of eta, mpmath truths, the measure, the regimes with the oracle's own error, and the
builders of the isolating models.  A plain helper module (imported explicitly by tests/test_logit_edges.py on the host and
tests/test_gpu_logit_edges.py on the device), after the pattern of tests/scalar_edges.py.

The device forms  lp = y eta - softplus(eta),  r = y - sigmoid(eta)  from e = exp(-|eta|); the oracle (oracle/csrc/oracle_logit.c,
oracle/ref_models.py `_logit_rows`) forms  lp = -softplus(-+eta),  r = y - expit(eta).

The measure (tests/scalar_edges.py):   e(a) = |a - T| / ( ulp(T) + ulp(eta) |dT/d eta| + c )
with T and dT/d eta from mpmath at `scalar_edges.PREC` bits (recomputed at twice the precision: the same doubles).  c = 0 except in
the CANCELLING regime y = 1, eta > 0, where the device's forms subtract two numbers that agree in almost every bit -- lp = eta -
(eta + log1p(e)), r = 1 - 1 / (1 + e) -- and the result carries one rounding of the larger operand however small the truth
(exp(-eta)) is: c = ulp(eta) for lp, 2^-53 for r.  The oracle's lp does not cancel there (its r does).

Regimes: y x sign of eta x {tiny: |eta| < 1e-8, core: up to 36.7 (e >= 2^-53), tail: up to 708 (e normal), denormal: up to 746
(e denormal), zero: beyond (e = 0, the clamp at 750 included)}.  `E_O` is the oracle's error per regime (the more accurate of the gcc
loop and the NumPy rows, each asserted by tests/test_logit_edges.py); the device must stay within FACTOR max(1, E_O) = 16 max(1, E_O).

Isolation for the rows node.  The benchmark's model (mu ~ N(0, 1), sigma ~ HalfNormal(1), z ~ N(0, 1)) with X[:, 0] = 1 and every
other entry 0 except one probe row per column d = 1 .. 7 with X[row, d] = 1, evaluated at mu = 0, log sigma = 0, z = 0 except
z[g_d, d] = eta_d: beta = z exactly, the probe row's eta is exactly eta_d, every other row's contribution to column d and the
prior's gradient at mu_d = 0 are exact zeros, so grad[mu_d] is that one row's r with no rounding in between.
"""
import functools
import math
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scalar_edges as se  # noqa: E402

from oracle import ref_models as rm  # noqa: E402
from pymc_amd.model_spec import ModelBuilder  # noqa: E402

PREC = se.PREC
FACTOR = se.FACTOR
LN2 = math.log(2.0)
D = 8
NPROBE = D - 1

# ---- the point table ------------------------------------------------------------------------------------------------------------
_PLAIN = [0.0, 5e-324, 2.0 ** -1022, 1e-300, 1e-17, 2.0 ** -53, 2.0 ** -52, 1e-8, 1e-3, 0.25, 0.5, 1.0, 2.0, 5.0, 10.0]
# (k +- 1/2) ln 2 and k ln 2: the reduction's rounding boundaries (k = rint(x log2 e)), the normal / denormal transition of e
# (1021 .. 1023), the last non-zero e (1074, 1075) and the clamp's k (750 log2 e = 1082.02)
_KS = [1, 2, 3, 10, 53, 54, 100, 1000, 1021, 1022, 1023, 1074, 1075, 1082]
_REDUCTION = [(k + h) * LN2 for k in _KS for h in (-0.5, 0.0, 0.5)]
_ORACLE_BRANCH = [37.0, 18.0, 33.3]          # oracle_logit.c `softplus` (-37 is the negative of the first)
_E_HALF_ULP = [36.7368, 37.43]                # e = 2^-53: 1 + e rounds to 1 from here on
_FAR = [40.0, 100.0, 300.0, 500.0, 700.0, 708.0, 708.3964, 709.0, 709.78, 710.0, 744.0, 745.0, 745.13, 746.0, 749.0, 750.0, 751.0, 800.0, 1e4, 1e300]
N_RANDOM = 120


def _random_points():
    rng = np.random.default_rng(20251)
    return np.concatenate([rng.uniform(-760.0, 760.0, N_RANDOM), rng.normal(0.0, 3.0, N_RANDOM),
                           np.exp(rng.uniform(math.log(1e-20), 0.0, N_RANDOM)) * rng.choice([-1.0, 1.0], N_RANDOM)])


def _table():
    out = {}
    for v in se.near(*(_PLAIN + _REDUCTION + _ORACLE_BRANCH + _E_HALF_ULP + _FAR)):
        for s in (1.0, -1.0):
            out[s * v + 0.0] = None          # (+ 0.0: one zero, the positive one)
    for v in _random_points():
        out[float(v)] = None
    pts = np.asarray(sorted(out), dtype="d")
    assert np.all(np.isfinite(pts))
    return pts


ETA = _table()
YS = (0, 1)
OUTPUTS = ("lp", "r")
CLASSES = (("tiny", 1e-8), ("core", 36.7), ("tail", 708.0), ("denormal", 746.0), ("zero", math.inf))


def regime_of(y, eta):
    a = abs(eta)
    name = "tiny" if a < 1e-8 else next(c for c, hi in CLASSES[1:] if a <= hi)
    return f"y{y}/{'neg' if eta < 0 else 'pos'}/{name}"          # (eta = 0 with the positive side: the device branches on eta >= 0)


REGIMES = tuple(f"y{y}/{s}/{c}" for y in YS for s in ("neg", "pos") for c, _ in CLASSES)


def cancelling(y, eta):
    return y == 1 and eta > 0


# ---- truths ---------------------------------------------------------------------------------------------------------------------
def _truth_mp(y, eta):
    """(lp, r, d r / d eta) in forms that do not cancel; d lp / d eta = r"""
    x = eta if isinstance(eta, mp.mpf) else mp.mpf(float(eta))
    # softplus(t) = max(t, 0) + log1p(exp(-|t|)): both terms of one sign
    l1p = mp.log1p(mp.exp(-abs(x)))
    if y:
        lp = -((-x if x < 0 else 0) + l1p)              # -softplus(-eta)
        r = 1 / (1 + mp.exp(x))                          # 1 - sigmoid(eta) = sigmoid(-eta)
    else:
        lp = -((x if x > 0 else 0) + l1p)               # -softplus(eta)
        r = -1 / (1 + mp.exp(-x))
    return lp, r, -1 / ((1 + mp.exp(-x)) * (1 + mp.exp(x)))


@functools.lru_cache(maxsize=None)
def truth(y, eta):
    """(lp, r, dr) in mpf at PREC bits; doubling the precision must return the same doubles"""
    with mp.workprec(PREC):
        a = _truth_mp(y, eta)
    with mp.workprec(2 * PREC):
        b = _truth_mp(y, eta)
    assert [se._to_double(v) for v in a] == [se._to_double(v) for v in b], (y, eta)
    return a


def floor_c(y, eta, output):
    if not cancelling(y, eta):
        return 0.0
    return se.ulp(eta) if output == "lp" else 2.0 ** -53


def denominator(y, eta, output):
    """ulp(T) + ulp(eta) |dT/d eta| + c, in mpf"""
    lp, r, dr = truth(y, eta)
    t, s = (lp, r) if output == "lp" else (r, dr)
    with mp.workprec(PREC):
        return mp.mpf(se.ulp(se._to_double(t))) + mp.mpf(se.ulp(eta)) * abs(s) + mp.mpf(floor_c(y, eta, output))


def measure(a, y, eta, output):
    if not math.isfinite(a):
        return math.inf
    t = truth(y, eta)[0 if output == "lp" else 1]
    with mp.workprec(PREC):
        return float(abs(mp.mpf(float(a)) - t) / denominator(y, eta, output))


def regime_errors(values, etas=None):
    """values: {(y, output): array over `etas` (default: ETA)} -> ({"regime/output": max e}, {"regime/output": (eta, value, e) of the worst point})"""
    etas = ETA if etas is None else etas
    worst, where = {}, {}
    for (y, o), col in values.items():
        for eta, a in zip(etas, col):
            k = f"{regime_of(y, float(eta))}/{o}"
            e = measure(float(a), y, float(eta), o)
            if e >= worst.get(k, -1.0):
                worst[k], where[k] = e, (float(eta), float(a), e)
    return worst, where


def max_abs_errors(values, etas=None):
    """{"regime/output": max |a - T|} (the cancelling regime's errors are stated as absolute ones)"""
    etas = ETA if etas is None else etas
    out = {}
    with mp.workprec(PREC):
        for (y, o), col in values.items():
            for eta, a in zip(etas, col):
                k = f"{regime_of(y, float(eta))}/{o}"
                out[k] = max(out.get(k, 0.0), float(abs(mp.mpf(float(a)) - truth(y, float(eta))[0 if o == "lp" else 1])))
    return out


def bound(key):
    return FACTOR * max(1.0, E_O[key])


# ---- the oracle, element by element: a model of ONE row (G = D = 1, X = [[1]]), whose rows term IS the row's lp and whose d / d mu
# IS its r (constrained values mu = 0, sigma = 1, z = eta: beta = 0 + 1 eta)
@functools.lru_cache(maxsize=None)
def one_row_spec(y):
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0, shape=1)
    sigma = m.HalfNormal("sigma", 1.0, shape=1)
    z = m.Normal("z", 0.0, 1.0, shape=(1, 1))
    m.HierLogitRows("y", np.ones((1, 1)), np.asarray([y], dtype="int8"), np.zeros(1, dtype="int32"), mu, sigma, z)
    return m.build()


def oracle_values(which, etas=None):
    """{(y, output): array} of the oracle's rows: `which` = "numpy" (ref_models._logit_rows) or "c" (the gcc loop of
    oracle/c_logit.CRowsSpecLogpGrad)"""
    etas = ETA if etas is None else etas
    out = {}
    for y in YS:
        spec = one_row_spec(y)
        if which == "c":
            from oracle import c_logit
            rows = c_logit.CRowsSpecLogpGrad(spec)._rows
        else:
            rows = rm._logit_rows
        lp, r = np.empty(len(etas)), np.empty(len(etas))
        with np.errstate(all="ignore"):
            for i, eta in enumerate(etas):
                lp[i], g = rows(spec, spec.logit_rows, np.asarray([0.0, 1.0, float(eta)]))
                r[i] = g[0]
        out[(y, "lp")], out[(y, "r")] = lp, r
    return out


# the oracle's error per regime (tests/test_logit_edges.py asserts for both: computed <= tabulated <= 1.5 computed + 1).  The two
# references differ in one regime: SciPy's expit returns 0 where exp(eta) is denormal (eta < -708.4: 2^43 denormal ulps from the
# truth), the gcc loop's e / (1 + e) keeps it.  Both have the same standing, so the device is held to the more accurate of the two.
E_O_C = {
    # E_O_C_TABLE_BEGIN
    "y0/neg/tiny/lp": 0.49, "y0/neg/tiny/r": 0.58, "y0/neg/core/lp": 0.66, "y0/neg/core/r": 0.79, "y0/neg/tail/lp": 0.015,
    "y0/neg/tail/r": 0.019, "y0/neg/denormal/lp": 0.5, "y0/neg/denormal/r": 0.5, "y0/neg/zero/lp": 0.22, "y0/neg/zero/r": 0.22,
    "y0/pos/tiny/lp": 0.71, "y0/pos/tiny/r": 0.57, "y0/pos/core/lp": 0.66, "y0/pos/core/r": 1.2, "y0/pos/tail/lp": 0.0079,
    "y0/pos/tail/r": 1, "y0/pos/denormal/lp": 1.5e-295, "y0/pos/denormal/r": 1.5e-292, "y0/pos/zero/lp": 4.6e-312,
    "y0/pos/zero/r": 4.7e-309, "y1/neg/tiny/lp": 0.71, "y1/neg/tiny/r": 0.79, "y1/neg/core/lp": 0.89, "y1/neg/core/r": 0.88,
    "y1/neg/tail/lp": 0.0079, "y1/neg/tail/r": 0.5, "y1/neg/denormal/lp": 1.5e-295, "y1/neg/denormal/r": 1.5e-292,
    "y1/neg/zero/lp": 4.6e-312, "y1/neg/zero/r": 4.7e-309, "y1/pos/tiny/lp": 0.54, "y1/pos/tiny/r": 0.38, "y1/pos/core/lp": 0.61,
    "y1/pos/core/r": 1.2, "y1/pos/tail/lp": 1.6e-18, "y1/pos/tail/r": 1, "y1/pos/denormal/lp": 2.2e-311,
    "y1/pos/denormal/r": 3e-292, "y1/pos/zero/lp": 9.2e-312, "y1/pos/zero/r": 9.4e-309,
    # E_O_C_TABLE_END
}
E_O_NUMPY = {
    # E_O_NUMPY_TABLE_BEGIN
    "y0/neg/tiny/lp": 0.53, "y0/neg/tiny/r": 1.4, "y0/neg/core/lp": 0.68, "y0/neg/core/r": 2, "y0/neg/tail/lp": 0.015,
    "y0/neg/tail/r": 0.021, "y0/neg/denormal/lp": 0.5, "y0/neg/denormal/r": 8.8e+12, "y0/neg/zero/lp": 0.22, "y0/neg/zero/r": 0.22,
    "y0/pos/tiny/lp": 0.71, "y0/pos/tiny/r": 0.57, "y0/pos/core/lp": 0.66, "y0/pos/core/r": 1.2, "y0/pos/tail/lp": 0.0079,
    "y0/pos/tail/r": 1, "y0/pos/denormal/lp": 1.5e-295, "y0/pos/denormal/r": 1.5e-292, "y0/pos/zero/lp": 4.6e-312,
    "y0/pos/zero/r": 4.7e-309, "y1/neg/tiny/lp": 0.71, "y1/neg/tiny/r": 0.66, "y1/neg/core/lp": 0.89, "y1/neg/core/r": 0.97,
    "y1/neg/tail/lp": 0.0079, "y1/neg/tail/r": 0.5, "y1/neg/denormal/lp": 1.5e-295, "y1/neg/denormal/r": 1.5e-292,
    "y1/neg/zero/lp": 4.6e-312, "y1/neg/zero/r": 4.7e-309, "y1/pos/tiny/lp": 0.51, "y1/pos/tiny/r": 0.38, "y1/pos/core/lp": 0.61,
    "y1/pos/core/r": 1.2, "y1/pos/tail/lp": 1.6e-18, "y1/pos/tail/r": 1, "y1/pos/denormal/lp": 2.2e-311,
    "y1/pos/denormal/r": 3e-292, "y1/pos/zero/lp": 9.2e-312, "y1/pos/zero/r": 9.4e-309,
    # E_O_NUMPY_TABLE_END
}
E_O = {k: min(E_O_C[k], E_O_NUMPY[k]) for k in E_O_C}


# ---- the isolating model of the rows node ---------------------------------------------------------------------------------------
def probe_places(G, rpg):
    """[(group, row in the group)] of the probes of columns 1 .. 7: different groups, the first and the last included; with 130 rows
    per group the places tests/test_gpu_rows_packed.py names (row 0, row 127, row 128 = the first row of the last tile, row 129 =
    the last valid row next to the masked padding), otherwise a group's first / last rows and rows inside it"""
    groups = [0, G - 1, 1, G // 2, G - 2, 2, 3]
    rows = [0, 129, 128, 127, 129, 0, 128] if rpg == 130 else [0, rpg - 1, rpg - 1, 0, 1, rpg - 2, rpg // 2]
    assert len(set(groups)) == NPROBE and G >= 7 and all(0 <= r < rpg for r in rows)
    return list(zip(groups, rows))


@functools.lru_cache(maxsize=None)
def rows_model(G, rpg, y_probe):
    """-> (spec, probe row indices [7]): the isolating model of the module docstring; the filler rows' y alternates"""
    N = G * rpg
    X = np.zeros((N, D))
    X[:, 0] = 1.0
    y = (np.arange(N) % 2).astype("int8")
    idx = []
    for d, (g, r) in enumerate(probe_places(G, rpg), start=1):
        X[g * rpg + r, d] = 1.0
        y[g * rpg + r] = y_probe
        idx.append(g * rpg + r)
    gidx = np.repeat(np.arange(G, dtype="int32"), rpg)
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0, shape=D)
    sigma = m.HalfNormal("sigma", 1.0, shape=D)
    z = m.Normal("z", 0.0, 1.0, shape=(G, D))
    m.HierLogitRows("y", X, y, gidx, mu, sigma, z)
    spec = m.build()
    assert [v.value_name for v in spec.vars] == ["mu", "sigma_log__", "z"] and spec.rows_order is None
    return spec, np.asarray(idx)


def rows_point(G, rpg, etas):
    """q of the isolating model with the probes at `etas` (up to 7; the rest at 0)"""
    q = np.zeros(2 * D + G * D)
    for d, ((g, _), eta) in enumerate(zip(probe_places(G, rpg), etas), start=1):
        q[2 * D + g * D + d] = eta
    return q


def chunks(etas=None, n=NPROBE):
    etas = ETA if etas is None else etas
    return [etas[i:i + n] for i in range(0, len(etas), n)]


def read_residuals(grad, n=NPROBE):
    return np.asarray(grad)[1:1 + n]          # grad[mu_d], d = 1 ..


# ---- the log-density in sum ------------------------------------------------------------------------------------------------------
def mp_normal_terms(z):
    """the two terms of log N(z | 0, 1): -z z / 2 and -log sqrt(2 pi)"""
    z = mp.mpf(float(z))
    return [-z * z / 2, -mp.log(2 * mp.pi) / 2]


@functools.lru_cache(maxsize=None)
def _mp_consts():
    with mp.workprec(PREC):
        return mp.log(2), -mp.log(2 * mp.pi) / 2, mp.log(2 / mp.pi) / 2


@functools.lru_cache(maxsize=None)
def mp_rows_model_logp(G, rpg, y_probe, etas):
    """(logp in mpf, sum_i den_i over the rows, sum_i |t_i| over all terms) of the isolating model at rows_point(G, rpg, etas)
    (`etas` a tuple): the priors (mu = 0; log sigma = 0: HalfNormal(1) at 1 and the Jacobian term log sigma = 0; z = 0 but for the
    probes) and every row (the fillers at eta = 0: -ln 2, denominator ulp(ln 2) -- ulp(0) |r| is below 1e-323) in mpmath"""
    with mp.workprec(PREC):
        ln2, lognorm, loghn = _mp_consts()
        etas = list(etas) + [0.0] * (NPROBE - len(etas))
        nfill = G * rpg - NPROBE
        terms = [lognorm] * (D + G * D) + [-mp.mpf(1) / 2, loghn] * D + [-ln2] * nfill
        terms += [-mp.mpf(float(e)) ** 2 / 2 for e in etas if e != 0.0]
        den = nfill * mp.mpf(se.ulp(LN2))
        for eta in etas:
            terms.append(truth(y_probe, float(eta))[0])
            den += denominator(y_probe, float(eta), "lp")
        return mp.fsum(terms), den, mp.fsum([abs(t) for t in terms])


DENSE_SEED = 77


def dense_case(G, rpg, span=40.0):
    """-> (spec, q, logp in mpf, sum_i den_i, sum_i |t_i|): the benchmark's model on rows of `models._hier_logit_data` at mu = 0,
    log sigma = 0 (beta = z exactly) and z = s beta*, beta* the coefficients the rows' y were drawn with and s the scale at which the
    largest |eta| is `span` -- y agrees with the sign of eta where |eta| is large, so the terms stay small next to a shift of every
    row.  eta_i is the exact dot product in mpmath; den_i = ulp(lp_i) + ulp(eta_i) |r_i| + c_i + D ulp(eta_i) |r_i|, the last
    term for the D roundings of the kernel's own eta.  (400 bits: the sum of some thousand terms to 1e-100 of itself.)"""
    from pymc_amd import models

    X, y, gidx = models._hier_logit_data(G, D, rpg, DENSE_SEED)
    rng = np.random.default_rng(DENSE_SEED)          # (the first two draws of `_hier_logit_data`: mu*, then beta*)
    mu_true = rng.normal(0, 0.5, size=D)
    beta = mu_true + 0.5 * rng.normal(size=(G, D))
    eta0 = np.einsum("nd,nd->n", X, beta[gidx])
    # beta* is a replay of the generator's draws: were their order to change, y would no longer follow these coefficients.  Rows
    # with |x . beta*| >= 2 were drawn with P(y = [eta > 0]) >= sigmoid(2) = 0.88; unrelated coefficients would agree on half.
    far = np.abs(eta0) >= 2.0
    assert far.sum() >= 100 and np.mean((y[far] != 0) == (eta0[far] > 0)) >= 0.85, "dense_case no longer replays models._hier_logit_data"
    z = beta * (span / np.max(np.abs(eta0)))
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0, shape=D)
    sigma = m.HalfNormal("sigma", 1.0, shape=D)
    zz = m.Normal("z", 0.0, 1.0, shape=(G, D))
    m.HierLogitRows("y", X, y, gidx, mu, sigma, zz)
    spec = m.build()
    q = np.concatenate([np.zeros(2 * D), z.ravel()])
    with mp.workprec(400):
        terms = []
        for _ in range(D):
            terms += mp_normal_terms(0.0) + [-mp.mpf(1) / 2, mp.log(2 / mp.pi) / 2]
        for v in z.ravel():
            terms += mp_normal_terms(v)
        den = mp.mpf(0)
        zm = [[mp.mpf(float(v)) for v in row] for row in z]
        for xi, yi, gi in zip(X, y, gidx):
            eta = mp.fsum([mp.mpf(float(a)) * b for a, b in zip(xi, zm[gi])])
            lp, r, _ = _truth_mp(int(yi), eta)
            ue = se.ulp(float(eta))
            den += mp.mpf(se.ulp(se._to_double(lp))) + (1 + D) * mp.mpf(ue) * abs(r) + (mp.mpf(ue) if yi and eta > 0 else 0)
            terms.append(lp)
        return spec, q, mp.fsum(terms), den, mp.fsum([abs(t) for t in terms])


# ---- the GLM node, Bernoulli family ----------------------------------------------------------------------------------------------
GLM_P = 64


@functools.lru_cache(maxsize=None)
def glm_model(P, y_value):
    """X = the P x P identity plus one all-zero row (P = 1: X = [[1]] alone), no intercept: eta_p = beta_p, grad[beta_p] = r_p"""
    X = np.eye(P) if P == 1 else np.concatenate([np.eye(P), np.zeros((1, P))])
    y = np.full(X.shape[0], float(y_value))
    m = ModelBuilder()
    b = m.Flat("beta", shape=P)
    m.GLM("y", X, b, y, family="bernoulli")
    return m.build()
