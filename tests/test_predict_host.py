"""Predictions at new data on the host: the NumPy restatement of the conditional moments (tests/predict_reference.py) gives the
moments `scipy.stats` gives, pymc_amd/csrc/predict.h -- the header k_pd_fold_* / k_pd_moments_* compile -- reproduces the restatement,
`model_spec.with_data` builds the spec the builder builds from the new data directly, and the fold recurrence is NumPy's mean,
population variance and logsumexp.

`tests/predict_check.cpp` is a stand-alone program around the header (system compiler, -Wall -Wextra -Werror, address and
undefined-behaviour sanitizers when they link); it is never loaded into Python.

Bars.  Restatement against SciPy, header against restatement: rtol 1e-12 (each formula is a few flops and at most one `exp`); the
+inf / NaN places are held to the table of the header, not to SciPy.  Bernoulli-logit edges: p (1 - p) against mpmath at 50 digits,
rounded to the nearest double (at eta = +-745 the true value, 0.57 of the smallest subnormal, has no double within 1e-12 of it: the
nearest one is the bar), rtol 1e-12.
"""
import dataclasses
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_reference as ref  # noqa: E402
from test_predictive_host import CASES, _floats, _tok  # noqa: E402

from pymc_amd import model_spec as ms  # noqa: E402
from pymc_amd.model_spec import ModelBuilder, data_inputs, with_data  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "predict_check.cpp")
INC = os.path.join(ROOT, "pymc_amd", "csrc")
RTOL = 1e-12
NAN, INF = math.nan, math.inf

# (label, dist, a1, a2, a3, scipy distribution or None, (mean, var) where the table of predict.h and not SciPy is the bar)
TABLE = [(c[0], c[1], c[2], c[3], c[4], c[5], None) for c in CASES]
SPECIAL = {"cauchy": (NAN, NAN), "halfcauchy": (INF, NAN), "studentt 0.8": (NAN, NAN)}
TABLE = [t[:6] + (SPECIAL.get(t[0]),) for t in TABLE]
TABLE += [(f"binomial {n} {p}", ref.D_BINOMIAL, float(n), p, 0.0, stats.binom(n, p), None) for n in (1, 7, 1000) for p in (0.0, 0.3, 1.0)]
TABLE += [
    ("studentt 1", ref.D_STUDENTT, 1.0, 0.3, 2.0, None, (NAN, NAN)),
    ("studentt 1.5", ref.D_STUDENTT, 1.5, 0.3, 2.0, None, (0.3, INF)),
    ("studentt 2", ref.D_STUDENTT, 2.0, 0.3, 2.0, None, (0.3, INF)),
    ("studentt 2.5", ref.D_STUDENTT, 2.5, 0.3, 2.0, stats.t(2.5, 0.3, 2.0), None),
    ("invgamma 0.5", ref.D_INVGAMMA, 0.5, 2.0, 0.0, None, (INF, NAN)),
    ("invgamma 1", ref.D_INVGAMMA, 1.0, 2.0, 0.0, None, (INF, NAN)),
    ("invgamma 1.5", ref.D_INVGAMMA, 1.5, 2.0, 0.0, None, (4.0, INF)),
    ("invgamma 2", ref.D_INVGAMMA, 2.0, 2.0, 0.0, None, (2.0, INF)),
    ("lognormal overflow", ref.D_LOGNORMAL, 700.0, 5.0, 0.0, None, (INF, INF)),
]
IDS = [t[0] for t in TABLE]

INVALID = [(ref.D_NORMAL, 0.0, -1.0, 0.0), (ref.D_NORMAL, 0.0, 0.0, 0.0), (ref.D_NORMAL, 0.0, NAN, 0.0), (ref.D_HALFNORMAL, -0.5, 0.0, 0.0),
           (ref.D_CAUCHY, 0.0, 0.0, 0.0), (ref.D_HALFCAUCHY, -1.0, 0.0, 0.0), (ref.D_STUDENTT, 4.0, 0.0, -1.0), (ref.D_STUDENTT, -1.0, 0.0, 1.0),
           (ref.D_EXPONENTIAL, 0.0, 0.0, 0.0), (ref.D_UNIFORM, 1.0, 0.5, 0.0), (ref.D_LOGNORMAL, 0.0, -2.0, 0.0), (ref.D_BERNOULLI, 1.5, 0.0, 0.0),
           (ref.D_BERNOULLI, -0.1, 0.0, 0.0), (ref.D_GAMMA, -1.0, 1.0, 0.0), (ref.D_GAMMA, 1.0, -1.0, 0.0), (ref.D_INVGAMMA, 1.0, 0.0, 0.0),
           (ref.D_LAPLACE, 0.0, -1.0, 0.0), (ref.D_POISSON, -0.5, 0.0, 0.0), (ref.D_POISSON, NAN, 0.0, 0.0), (ref.D_BERNOULLI_LOGIT, NAN, 0.0, 0.0),
           (ref.D_BINOMIAL, -1.0, 0.5, 0.0), (ref.D_BINOMIAL, 5.0, 1.5, 0.0), (ref.D_BINOMIAL, 5.0, NAN, 0.0), (ref.D_BETA, 0.0, 1.0, 0.0)]


def _same(got, want, label=""):
    got, want = np.asarray(got, dtype="float64"), np.asarray(want, dtype="float64")
    assert got.shape == want.shape, label
    assert np.array_equal(np.isnan(got), np.isnan(want)), (label, got, want)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), (label, got, want)
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=0.0, err_msg=label)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(TABLE)), ids=IDS)
def test_the_restatement_has_the_moments_of_the_family(case):
    label, dist, a1, a2, a3, sp, special = TABLE[case]
    m, v = ref.moments(dist, a1, a2, a3)
    if special is not None:
        _same([m, v], special, label)
        return
    want = (float(sp.mean()), float(sp.var()))
    assert np.all(np.isfinite(want)), label
    print(label, "relative differences", abs(m - want[0]) / max(abs(want[0]), 1e-300), abs(v - want[1]) / max(abs(want[1]), 1e-300))
    _same([m, v], want, label)


def test_the_restatement_of_the_mixture_has_its_moments():
    mu, sg, w = np.array([-2.0, 0.5, 3.0]), np.array([0.5, 1.0, 0.7]), np.array([0.2, 0.5, 0.3])
    m, v = ref.mixture_moments(mu, sg, w)
    second = float(np.sum(w * (sg ** 2 + mu ** 2)))
    _same([m, v], [float(np.sum(w * mu)), second - float(np.sum(w * mu)) ** 2])


def test_bernoulli_logit_variance_at_the_edges_does_not_cancel():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    for eta in (40.0, -40.0, 745.0, -745.0):
        e = mp.exp(-abs(mp.mpf(eta)))
        true = e / (1 + e) ** 2
        want = float(true)
        m, v = ref.moments(ref.D_BERNOULLI_LOGIT, eta)
        print(eta, "p (1 - p)", float(v), "mpmath", mp.nstr(true, 20))
        assert want > 0.0 and float(v) > 0.0
        np.testing.assert_allclose(float(v), want, rtol=RTOL, atol=0.0)
        np.testing.assert_allclose(float(m), float(1 / (1 + mp.exp(-mp.mpf(eta)))), rtol=RTOL, atol=0.0)


def test_refused_families_are_refused():
    for dist in (ref.D_TRUNCNORMAL, ref.D_POTENTIAL, ref.D_DERIVED, 19, -1):
        with pytest.raises(ValueError, match="refused"):
            ref.moments(dist, 0.0, 1.0)


# ---- the header ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(INC, "predict.h")), "pymc_amd/csrc/predict.h is missing"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    out = str(tmp_path_factory.mktemp("predict") / "predict_check")
    base = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + INC, SRC, "-o", out]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return out


def _run(exe, req, code=0):
    r = subprocess.run([exe], input=req, capture_output=True, text=True)
    assert r.returncode == code, (r.returncode, r.stderr)
    return r.stdout


_values = _floats      # (hex floats, nan, inf, -inf)


def _mom_req(dist, a1, a2, a3):
    return f"mom {dist} {_tok(a1)} {_tok(a2)} {_tok(a3)}\n"


def test_the_header_reproduces_the_restatement(exe):
    rows = [(t[1], t[2], t[3], t[4]) for t in TABLE] + INVALID
    rows += [(ref.D_BERNOULLI_LOGIT, eta, 0.0, 0.0) for eta in (40.0, -40.0, 745.0, -745.0, 800.0, -800.0, 0.0)]
    got = _values(_run(exe, "".join(_mom_req(*r) for r in rows))).reshape(-1, 2)
    want = np.array([ref.moments(*r) for r in rows], dtype="float64")
    assert np.all(np.isnan(want[len(TABLE): len(TABLE) + len(INVALID)]))
    _same(got, want)
    edge = got[len(TABLE) + len(INVALID):]
    assert np.all(edge[:4, 1] > 0.0), "p (1 - p) must not be 0 where the true value is representable"


def test_the_header_reproduces_the_mixture(exe):
    rng = np.random.default_rng(5)
    for K in (1, 3, 16):
        mu, sg = rng.normal(size=K) * 2.0, 0.5 + rng.random(K)
        w = rng.dirichlet(np.ones(K))
        got = _values(_run(exe, f"mix {K} " + " ".join(_tok(v) for v in np.concatenate([mu, sg, w])) + "\n"))
        _same(got, ref.mixture_moments(mu, sg, w))


def test_the_program_refuses_what_is_out_of_scope(exe):
    for dist in (ref.D_TRUNCNORMAL, ref.D_POTENTIAL, ref.D_DERIVED, 19, -1):
        _run(exe, _mom_req(dist, 0.0, 1.0, 0.0), code=4)
    _run(exe, "mom 0 0x1p0 1.0x 0\n", code=2)
    _run(exe, "what\n", code=2)


# ---- the fold -----------------------------------------------------------------------------------------------------------------------
def _fold_matrix():
    """[S, N] values of m, v and lp: plain columns, and columns with -inf, nothing but -inf, NaN and +inf in them"""
    rng = np.random.default_rng(11)
    S, N = 19, 9
    m, v, lp = rng.normal(size=(S, N)) * 3.0 + 1.0, rng.random((S, N)) + 0.1, rng.normal(size=(S, N)) * 4.0 - 3.0
    lp[[2, 7], 1] = -np.inf
    lp[:, 2] = -np.inf
    lp[5, 3] = np.nan
    lp[4, 4] = np.inf
    lp[0, 5] = -np.inf          # (the first value)
    lp[:, 6] -= 800.0           # (exp of the values themselves underflows)
    m[3, 3], v[9, 4] = np.nan, np.nan
    m[6, 5], v[[1, 12], 6] = np.inf, np.inf
    v[0, 7] = np.inf
    return m, v, lp


def _hold_fold(state, m, v, lp):
    want = ref.predict(m, v, lp)
    mean, vb, vw, lpd = ref.read(state)
    _same(mean, want["mean"], "mean")
    _same(vb, want["var_between"], "var_between")
    _same(vw, want["var_within"], "var_within")
    _same(lpd, want["lpd_i"], "lpd")
    assert np.isneginf(lpd[2]) and np.isnan(lpd[3]) and lpd[4] == np.inf and np.isfinite(lpd[[0, 1, 5, 6]]).all()
    assert np.isnan(mean[3]) and np.isnan(vw[4]) and mean[5] == np.inf and vw[6] == np.inf and vw[7] == np.inf


def test_the_fold_recurrence_is_numpy_on_the_matrix():
    m, v, lp = _fold_matrix()
    state = ref.fold(m, v, lp)
    _hold_fold(state, m, v, lp)
    # any split over calls continues the same recurrence
    part = ref.fold(m[12:], v[12:], lp[12:], state=ref.fold(m[5:12], v[5:12], lp[5:12], state=ref.fold(m[:5], v[:5], lp[:5])))
    for a, b in zip(state, part):
        assert np.array_equal(a, b, equal_nan=True)
    assert ref.read(ref.fold(m, v), with_lp=False)[3] is None


def test_the_header_folds_as_the_restatement(exe):
    m, v, lp = _fold_matrix()
    req = "".join(f"fold {m.shape[0]} 1 " + " ".join(f"{_tok(m[s, i])} {_tok(v[s, i])} {_tok(lp[s, i])}" for s in range(m.shape[0])) + "\n" for i in range(m.shape[1]))
    got = _values(_run(exe, req)).reshape(m.shape[1], 7)
    state = ref.fold(m, v, lp)
    for k in range(5):
        _same(got[:, k], state[k], f"accumulator row {k}")
    assert np.all(got[:, 5] == m.shape[0])
    _same(got[:, 6], ref.read(state)[3], "lpd")
    _hold_fold(tuple(got[:, k] for k in range(5)) + (float(m.shape[0]),), m, v, lp)


def test_predict_from_accumulators_is_the_numpy_summary():
    from pymc_amd import predictive

    m, v, lp = _fold_matrix()
    keep = [0, 1, 6]
    m, v, lp = m[:, keep], v[:, keep], lp[:, keep]
    v[:, 2] = np.abs(v[:, 0])
    want = ref.predict(m, v, lp)
    out = predictive.predict_from_accumulators(*ref.read(ref.fold(m, v, lp)), n_draws=m.shape[0])
    for k in ("mean", "var_between", "var_within", "sd", "lpd_i", "elpd", "se"):
        np.testing.assert_allclose(out[k], want[k], rtol=1e-12, err_msg=k)
    assert out["n_samples"] == m.shape[0] and out["n_data_points"] == 3
    # the law of total variance: the variance of the mixture of the draws, computed directly from its second moment
    total = (v + m * m).mean(axis=0) - m.mean(axis=0) ** 2
    np.testing.assert_allclose(out["sd"] ** 2, total, rtol=1e-10)
    bare = predictive.predict_from_accumulators(*ref.read(ref.fold(m, v))[:3], None, n_draws=m.shape[0])
    assert "lpd_i" not in bare and "elpd" not in bare
    assert "lpd_i" not in predictive.predict_from_accumulators(*ref.read(ref.fold(m, v, lp)), n_draws=m.shape[0], pointwise=False)


# ---- with_data against a fresh build -----------------------------------------------------------------------------------------------
def _equal(a, b, path="spec"):
    if dataclasses.is_dataclass(a) and not isinstance(a, type):
        assert type(a) is type(b), path
        for f in dataclasses.fields(a):
            _equal(getattr(a, f.name), getattr(b, f.name), f"{path}.{f.name}")
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), path
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, f"{path}[{i}]")
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _equal(a[k], b[k], f"{path}[{k!r}]")
    else:
        assert a == b or (a != a and b != b), (path, a, b)


def _glm(family, X, y):
    m = ModelBuilder()
    alpha = m.Normal("alpha", 0.0, 5.0)
    beta = m.Normal("beta", 0.0, 1.0, shape=X.shape[1])
    sg = m.HalfNormal("sigma", 1.0) if family == "normal" else 1.0
    m.GLM("y", X, beta, y, family=family, intercept=alpha, sigma=sg)
    return m.build()


def _glm_data(family, N, P, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, P))
    y = rng.normal(size=N) if family == "normal" else (rng.random(N) < 0.5).astype("float64") if family == "bernoulli" else rng.poisson(2.0, N).astype("float64")
    return X, y


@pytest.mark.parametrize("family", ["normal", "bernoulli", "poisson"])
def test_with_data_glm_is_the_fresh_build(family):
    train = _glm(family, *_glm_data(family, 40, 3, 1))
    Xn, yn = _glm_data(family, 17, 3, 2)
    new = with_data(train, {"y": {"X": Xn, "y": yn}})
    _equal(new, _glm(family, Xn, yn))
    assert new.n == train.n and new.point_map_info == train.point_map_info and train.glm_rows.X.shape == (40, 3)
    bare = with_data(train, {"y": {"X": Xn}})
    want = _glm(family, Xn, np.zeros(17))
    want.predict_no_y = ("y",)
    _equal(bare, want)
    assert data_inputs(train) == {"y": {"X": 3, "y": None}}
    for bad in ({"X": Xn[:, :2]}, {"X": Xn, "y": yn[:5]}, {"y": yn}):
        with pytest.raises(ValueError, match="'y'"):
            with_data(train, {"y": bad})
    with pytest.raises(KeyError, match="nope"):
        with_data(train, {"nope": {"X": Xn}})


def _logit(X, y, g, G):
    D = X.shape[1]
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0, shape=D)
    sigma = m.HalfNormal("sigma", 1.0, shape=D)
    z = m.Normal("z", 0.0, 1.0, shape=(G, D))
    m.HierLogitRows("y", X, y, g, mu, sigma, z)
    return m.build()


def test_with_data_logit_rows_unsorted_with_an_empty_group_is_the_fresh_build():
    from pymc_amd import loglik, models

    rng = np.random.default_rng(3)
    G, D = 4, 3
    train = models.hier_logit(G=G, D=D, rows_per_group=6)
    M = 11
    Xn, yn = rng.normal(size=(M, D)), (rng.random(M) < 0.5).astype("int8")
    gn = rng.choice([0, 1, 3], size=M).astype("int32")     # group 2 has no new row; the rows are not sorted
    assert np.any(np.diff(gn) < 0)
    new = with_data(train, {"y": {"X": Xn, "group_idx": gn, "y": yn}})
    _equal(new, _logit(Xn, yn, gn, G))
    assert new.n == train.n and train.rows_order is None and train.logit_rows.X.shape == (G * 6, D)
    assert np.array_equal(loglik.caller_order(new, ms.LL_LOGIT_ROWS, new.logit_rows.y.astype("float64")), yn)
    bare = with_data(train, {"y": {"X": Xn, "group_idx": gn}})
    want = _logit(Xn, np.zeros(M, dtype="int8"), gn, G)
    want.predict_no_y = ("y",)
    _equal(bare, want)
    # rows passed sorted keep no order
    o = np.argsort(gn, kind="stable")
    assert with_data(train, {"y": {"X": Xn[o], "group_idx": gn[o]}}).rows_order is None
    assert data_inputs(train) == {"y": {"X": D, "group_idx": G, "y": None}}
    for bad in ({"X": Xn[:, :2], "group_idx": gn}, {"X": Xn, "group_idx": gn + 1}, {"X": Xn, "group_idx": gn[:3]}, {"X": Xn}, {"X": Xn, "group_idx": gn, "y": yn[:2]}):
        with pytest.raises(ValueError, match="'y'"):
            with_data(train, {"y": bad})


def _poisson(x, exposure, y):
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    b = m.Normal("b", 0.0, 1.0)
    m.Poisson("counts", m.as_expr(exposure) * m.math.exp(a + b * m.as_expr(x)), observed=y)
    return m.build()


def test_with_data_poisson_factor_with_exposure_is_the_fresh_build():
    rng = np.random.default_rng(4)
    mk = lambda n: (rng.normal(size=n), rng.uniform(0.5, 2.0, size=n), rng.poisson(2.0, n).astype("float64"))   # noqa: E731
    train = _poisson(*mk(30))
    x, e, y = mk(13)
    ins = data_inputs(train)["counts"]
    assert len(ins["data"]) == 2 and ins["observed"] is None
    ex_id, x_id = ins["data"]          # the order the argument first reads them: exposure, then x
    assert np.array_equal(train.data[ex_id], train.data[ex_id]) and train.data[x_id].size == 30
    new = with_data(train, {"counts": {"data": {ex_id: e, x_id: x}, "observed": y}})
    _equal(new, _poisson(x, e, y))
    assert new.factors[-1].size == 13 and train.factors[-1].size == 30 and new.n == train.n
    bare = with_data(train, {"counts": {"data": {ex_id: e, x_id: x}}})
    want = _poisson(x, e, np.zeros(13))
    want.predict_no_y = ("counts",)
    _equal(bare, want)
    with pytest.raises(ValueError, match="'counts'.*must be given"):
        with_data(train, {"counts": {"data": {x_id: x}, "observed": y}})
    with pytest.raises(ValueError, match="'counts'.*one new length"):
        with_data(train, {"counts": {"data": {ex_id: e[:5], x_id: x}, "observed": y[:5]}})
    with pytest.raises(ValueError, match="'counts'.*'observed' has"):
        with_data(train, {"counts": {"data": {ex_id: e, x_id: x}, "observed": y[:5]}})
    with pytest.raises(ValueError, match="'counts'.*does not read"):
        with_data(train, {"counts": {"data": {ex_id: e, x_id: x, 99: x}}})


def _binomial(x, n, y):
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    m.Binomial("k", n, m.math.sigmoid(a + m.as_expr(x)), observed=y)
    return m.build()


def test_with_data_binomial_factor_with_a_vector_n_is_the_fresh_build():
    rng = np.random.default_rng(5)

    def mk(size):
        n = rng.integers(1, 20, size=size).astype("float64")
        return rng.normal(size=size), n, np.floor(rng.random(size) * (n + 1))

    train = _binomial(*mk(12))
    x, n, y = mk(7)
    ids = data_inputs(train)["k"]["data"]
    assert len(ids) == 2
    n_id, x_id = ids
    new = with_data(train, {"k": {"data": {n_id: n, x_id: x}, "observed": y}})
    _equal(new, _binomial(x, n, y))
    bare = with_data(train, {"k": {"data": {n_id: n, x_id: x}}})
    want = _binomial(x, n, np.zeros(7))
    want.predict_no_y = ("k",)
    _equal(bare, want)
    # a constant n: the coefficient follows the new observed values alone
    train_c = _binomial(rng.normal(size=12), 10.0, np.floor(rng.random(12) * 11))
    (xc_id,) = data_inputs(train_c)["k"]["data"]
    _equal(with_data(train_c, {"k": {"data": {xc_id: x}, "observed": np.minimum(y, 10.0)}}), _binomial(x, 10.0, np.minimum(y, 10.0)))


def _schools(sigma, y):
    m = ModelBuilder()
    eta = m.Normal("eta", 0.0, 1.0, shape=8)
    mu = m.Normal("mu", 0.0, 1e6)
    tau = m.HalfCauchy("tau", 25.0)
    m.Normal("obs", mu + tau * eta, sigma, observed=y)
    return m.build()


def test_with_data_eight_schools_with_new_sigma_is_the_fresh_build():
    from pymc_amd import models

    train = models.eight_schools()
    sigma, y = np.arange(8) + 5.0, np.linspace(-3, 20, 8)
    (s_id,) = data_inputs(train)["obs"]["data"]
    _equal(with_data(train, {"obs": {"data": {s_id: sigma}, "observed": y}}), _schools(sigma, y))
    # the school effects are a variable read element by element: eight rows, no more
    with pytest.raises(ValueError, match="'obs'.*'eta'"):
        with_data(train, {"obs": {"data": {s_id: np.ones(9)}, "observed": np.ones(9)}})


def test_with_data_scalar_parameters_take_the_length_from_observed():
    def build(y):
        m = ModelBuilder()
        mu = m.Normal("mu", 0.0, 1.0)
        s = m.HalfNormal("s", 1.0)
        m.Normal("y", mu, s, observed=y)
        return m.build()

    rng = np.random.default_rng(6)
    train, y = build(rng.normal(size=9)), rng.normal(size=4)
    assert data_inputs(train) == {"y": {"data": [], "observed": None}}
    _equal(with_data(train, {"y": {"observed": y}}), build(y))
    with pytest.raises(ValueError, match="'y'.*nothing sets the new length"):
        with_data(train, {"y": {}})


def test_with_data_marginal_mixture():
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 10.0, shape=3)
    m.NormalMixture("y", np.array([0.2, 0.5, 0.3]), mu, m.HalfNormal("sigma", 2.0, shape=3), np.linspace(-3, 3, 50))
    train = m.build()
    assert train.mixture_rows.assign is None
    name = train.mixture_rows.name
    y = np.linspace(-2, 2, 7)
    new = with_data(train, {name: {"y": y}})
    want = dataclasses.replace(train, mixture_rows=dataclasses.replace(train.mixture_rows, y=y))
    _equal(new, want)
    assert train.mixture_rows.y.size == 50 and data_inputs(train)[name] == {"y": None}
    with pytest.raises(ValueError, match=repr(name)):
        with_data(train, {name: {}})


def test_with_data_refusals_name_the_variable():
    from pymc_amd import models, predictive

    # extra inputs / the conditional mixture: `loglik.refusal`'s reasons
    cond = models.normal_mixture(N=50, K=3, form="node")
    with pytest.raises(ValueError, match="extra inputs"):
        with_data(cond, {cond.mixture_rows.name: {"y": np.zeros(3)}})
    cond.extra = {}
    with pytest.raises(ValueError, match=repr(cond.mixture_rows.name) + ".*conditional mixture"):
        with_data(cond, {cond.mixture_rows.name: {"y": np.zeros(3)}})
    # a linear-predictor matrix under an observed factor
    rng = np.random.default_rng(7)
    m = ModelBuilder()
    beta = m.Normal("beta", 0.0, 1.0, shape=3)
    m.Normal("y_lin", m.dot(rng.normal(size=(6, 3)), beta), 1.0, observed=rng.normal(size=6))
    with pytest.raises(ValueError, match="'y_lin'.*linear-predictor"):
        with_data(m.build(), {"y_lin": {"observed": np.zeros(4)}})
    # a vector another factor reads, a Deterministic over replaced data
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    x = m.as_expr(rng.normal(size=5))
    m.Normal("y1", a * x, 1.0, observed=rng.normal(size=5))
    m.Normal("y2", a + x, 1.0, observed=rng.normal(size=5))
    spec = m.build()
    (x_id,) = data_inputs(spec)["y1"]["data"]
    with pytest.raises(ValueError, match="'y1'.*also read by factor 'y2'"):
        with_data(spec, {"y1": {"data": {x_id: np.zeros(3)}, "observed": np.zeros(3)}})
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    x = m.as_expr(rng.normal(size=5))
    m.Deterministic("fit", a * x)
    m.Normal("y1", a * x, 1.0, observed=rng.normal(size=5))
    spec = m.build()
    (x_id,) = data_inputs(spec)["y1"]["data"]
    with pytest.raises(ValueError, match="'y1'.*Deterministic 'fit'"):
        with_data(spec, {"y1": {"data": {x_id: np.zeros(3)}, "observed": np.zeros(3)}})
    # a gather whose new index leaves the variable
    m = ModelBuilder()
    g = m.Normal("g", 0.0, 1.0, shape=4)
    m.Normal("y_g", g[np.array([0, 1, 3, 3, 2])], 1.0, observed=rng.normal(size=5))
    spec = m.build()
    (i_id,) = data_inputs(spec)["y_g"]["data"]
    assert with_data(spec, {"y_g": {"data": {i_id: np.array([3.0, 0.0])}}}).factors[-1].size == 2
    with pytest.raises(ValueError, match="'y_g'.*leaves variable 'g'"):
        with_data(spec, {"y_g": {"data": {i_id: np.array([4.0, 0.0])}}})
    # the families without moments
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    m.TruncatedNormal("y_t", a, 1.0, lower=0.0, observed=np.ones(3))
    spec = m.build()
    assert "TruncatedNormal" in predictive.predict_refusal(spec) and "y_t" in predictive.predict_refusal(spec)
    with pytest.raises(ValueError, match="predictions refused.*TruncatedNormal"):
        predictive.predict(spec, np.zeros((1, 2, spec.n)), {"y_t": {"observed": np.ones(2)}})


def test_the_calls_refuse_a_null_handle():
    import ctypes as C

    import __graft_entry__ as g

    g.build_engine()
    from pymc_amd import _lib

    lib = _lib.load()
    out = np.full(4, 7.0)
    n = C.c_int64(-1)
    assert lib.nuts_model_predict_moments(None, 0, 0, _lib.dptr(out), 1, _lib.dptr(out), None) == _lib.NUTS_E_ARG
    assert not lib.nuts_pred_create(None, 0, 0, 1)
    assert lib.nuts_pred_update(None, _lib.dptr(out), 1) == _lib.NUTS_E_ARG
    assert lib.nuts_pred_read(None, None, None, None, None, C.byref(n)) == _lib.NUTS_E_ARG and n.value == -1
    lib.nuts_pred_destroy(None)
    assert np.all(out == 7.0)
