"""Power-scaling sensitivity on the host: the NumPy restatement (tests/psens_reference.py) against its own 200-bit form, and
pymc_amd/csrc/psens.h -- the header k_psens and k_psens_weights compile -- against the restatement.

`tests/psens_check.cpp` is a stand-alone program around the header (system compiler, -Wall -Wextra -Werror, address and
undefined-behaviour sanitizers when they link); it is never loaded into Python.
"""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prior_models as pm_  # noqa: E402
import psens_reference as ps  # noqa: E402
import psis_reference as pr  # noqa: E402

from pymc_amd import model_spec as ms  # noqa: E402
from pymc_amd import models, sensitivity  # noqa: E402
from pymc_amd.model_spec import ModelBuilder  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "psens_check.cpp")
INC = os.path.join(ROOT, "pymc_amd", "csrc")
EPS = np.finfo("float64").eps


def synthetic(S, seed, kind="normal"):
    """(x, lc): draws of one parameter and a component's log-density that depends on them, so the weights tilt the ECDF"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(S)
    if kind == "ties":
        x = (rng.integers(0, 1000, size=S) % 7).astype("float64")
    lc = -0.5 * (x - 1.0) ** 2 * 3.0 + 0.1 * rng.standard_normal(S)
    return x, lc


def both_weights(lc, delta=0.01):
    a_lo, a_hi = ps.alphas(delta)
    return ps.weights(lc, a_lo)[0], ps.weights(lc, a_hi)[0]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_uniform_weights_give_zero_up_to_rounding():
    """Q = cumsum(1 / S) is P up to S eps / 2; D is of second order in P - Q and its sums carry a few eps of their own: S eps"""
    for S in (2, 3, 100, 1000):
        x = np.random.default_rng(S).standard_normal(S)
        d = ps.distance_both(x, np.full(S, 1.0 / S))
        print("uniform weights S", S, "D", d)
        assert 0.0 <= d <= S * EPS


def test_one_hot_weights_exercise_the_log2_guard():
    """all the weight on the smallest draw: Q = 1 everywhere; on the largest: Q = 0 everywhere (L(0) = 0); mirrored, each is the other"""
    for S in (2, 5, 100):
        x = np.random.default_rng(10 + S).standard_normal(S)
        for at in (int(np.argmin(x)), int(np.argmax(x)), S // 2):
            w = np.zeros(S)
            w[at] = 1.0
            for sign in (1.0, -1.0):
                d, t = ps.distance(sign * x, w), ps.distance_mp(sign * x, w)
                assert math.isfinite(d) and 0.0 < d <= 1.0 and abs(d - t) <= 64 * EPS, (S, at, sign, d, t)
    # the closed form at S = 2, the weight on the smaller draw: P = 1/2, Q = 1, M = 3/4
    d = ps.distance(np.array([0.0, 1.0]), np.array([1.0, 0.0]))
    pq = 0.5 * (math.log2(0.5) - math.log2(0.75)) + 0.5 / (2 * math.log(2))
    qp = -math.log2(0.75) - 0.5 / (2 * math.log(2))
    assert abs(d - (pq + qp) / 1.5) <= 4 * EPS


def test_ties_and_constant_parameters():
    x, lc = synthetic(500, 3, "ties")
    w_lo, w_hi = both_weights(lc)
    for w in (w_lo, w_hi):
        d, t = ps.distance_both(x, w), ps.distance_both(x, w, ps.distance_mp)
        assert abs(d - t) <= 64 * EPS, (d, t)
    assert math.isnan(ps.distance(np.full(50, 2.5), np.full(50, 0.02)))
    assert all(math.isnan(v) for v in ps.psens_one(np.full(50, 2.5), w_lo[:50], w_hi[:50]))
    bad = x.copy()
    bad[7] = np.inf
    assert all(math.isnan(v) for v in ps.psens_one(bad, w_lo, w_hi))
    # a permutation of the draws with their weights moves D by rounding only
    p = np.random.default_rng(0).permutation(500)
    assert abs(ps.distance(x[p], w_lo[p]) - ps.distance(x, w_lo)) <= 64 * EPS


def test_weights_follow_the_definition():
    x, lc = synthetic(100, 4)
    for alpha in ps.alphas():
        w, khat = ps.weights(lc, alpha)
        assert abs(w.sum() - 1.0) <= 100 * EPS and math.isfinite(khat)
        # against the raw ratios: the bulk of the draws keeps them
        raw = np.exp((alpha - 1.0) * lc - np.max((alpha - 1.0) * lc))
        raw /= raw.sum()
        assert np.median(np.abs(w / raw - 1.0)) < 1e-3
    w, khat = ps.weights(lc[:16], 1.01)                 # a tail of 4: nothing is smoothed
    raw = np.exp(0.01 * lc[:16] - np.max(0.01 * lc[:16]))
    assert pr.tail_len(16) == 4 and khat == math.inf
    np.testing.assert_allclose(w, raw / raw.sum(), rtol=1e-14)
    lc2 = lc.copy()
    lc2[5] = -np.inf
    w, khat = ps.weights(lc2, 1.01)
    assert np.all(np.isnan(w)) and math.isnan(khat)


def test_the_diagnosis_table():
    nan = math.nan
    prior = [0.2, 0.2, 0.01, 0.01, nan, 0.2, 0.05, 0.06]
    lik = [0.3, 0.01, 0.3, 0.01, 0.3, nan, 0.3, 0.05]
    want = ["prior-data conflict", "strong prior / weak likelihood", "-", "-", "-", "-", "-", "strong prior / weak likelihood"]
    assert sensitivity.diagnose(prior, lik) == want == ps.diagnose(prior, lik)


def _conjugate(m0, s0, S=400, seed=1):
    """y_i ~ Normal(mu, 1), 20 observations centred at 0, mu ~ Normal(m0, s0): exact posterior draws, log-prior, log-likelihood"""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(20)
    y -= y.mean()
    prec = 1.0 / s0 ** 2 + 20.0
    mu = (m0 / s0 ** 2 + y.sum()) / prec + rng.standard_normal(S) / math.sqrt(prec)
    lp = -0.5 * ((mu - m0) / s0) ** 2 - math.log(s0) - 0.5 * math.log(2 * math.pi)
    ll = np.sum(-0.5 * (y[None, :] - mu[:, None]) ** 2 - 0.5 * math.log(2 * math.pi), axis=1)
    return mu, lp, ll


def test_the_reference_lands_on_the_intended_side_for_the_two_conjugate_models():
    """what tests/test_gpu_psens.py asks of the device end to end, first on the host with exact posterior draws: room to spare"""
    mu, lp, ll = _conjugate(10.0, 0.05)
    p, l = ps.psens_arrays(mu[:, None], lp)["sensitivity"][0], ps.psens_arrays(mu[:, None], ll)["sensitivity"][0]
    print("conflict model: prior", p, "likelihood", l)
    assert p > 0.2 and l > 0.2 and ps.diagnose([p], [l]) == ["prior-data conflict"]
    mu, lp, ll = _conjugate(0.0, 100.0)
    p, l = ps.psens_arrays(mu[:, None], lp)["sensitivity"][0], ps.psens_arrays(mu[:, None], ll)["sensitivity"][0]
    print("vague prior: prior", p, "likelihood", l)
    assert p < 0.0125 and ps.diagnose([p], [l]) == ["-"]


# ---- the header ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(INC, "psens.h")), "pymc_amd/csrc/psens.h is missing"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    out = str(tmp_path_factory.mktemp("psens") / "psens_check")
    base = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + INC, SRC, "-o", out]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return out


def _tok(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("inf" if v == math.inf else ("-inf" if v == -math.inf else v.hex()))


def _run(exe, requests):
    req = "".join(" ".join(_tok(v) for v in r) + "\n" for r in requests)
    r = subprocess.run([exe], input=req, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return [float("nan") if w in ("nan", "-nan") else float.fromhex(w) if "x" in w else float(w) for w in r.stdout.split()]


def _cases():
    out = []
    for S in (2, 3, 17, 255, 256, 257, 1000):
        x, lc = synthetic(S, S)
        out.append((f"normal S={S}", x, *both_weights(lc)))
    x, lc = synthetic(300, 8, "ties")
    out.append(("ties", x, *both_weights(lc)))
    x = np.random.default_rng(9).standard_normal(50)
    hot = np.zeros(50)
    hot[int(np.argmax(x))] = 1.0
    cold = np.zeros(50)
    cold[int(np.argmin(x))] = 1.0
    out.append(("one-hot", x, hot, cold))
    out.append(("uniform", x, np.full(50, 0.02), np.full(50, 0.02)))
    return out


def test_the_header_reproduces_the_distance(exe):
    cases = _cases()
    got = _run(exe, [[1, x.size, *x, *w] for _, x, w, _ in cases])
    worst = 0.0
    for k, (label, x, w, _) in enumerate(cases):
        for d, ref, truth in ((got[2 * k], ps.distance(x, w), ps.distance_mp(x, w)), (got[2 * k + 1], ps.distance(-x, w), ps.distance_mp(-x, w))):
            print(label, "header", d, "restatement", ref, "200-bit", truth)
            worst = max(worst, abs(d - truth))
            # both are float64 evaluations of the same sums in (nearly) the same order: S eps covers the scan's and the sums' rounding
            assert abs(d - ref) <= x.size * EPS and abs(d - truth) <= x.size * EPS, (label, d, ref, truth)
    print("header: worst |D - truth|", worst)
    const = _run(exe, [[1, 4, 2.5, 2.5, 2.5, 2.5, 0.25, 0.25, 0.25, 0.25]])
    assert all(math.isnan(v) for v in const)


def test_the_header_reproduces_the_columns(exe):
    cases = _cases()
    got = _run(exe, [[2, x.size, 0.01, *x, *w_lo, *w_hi] for _, x, w_lo, w_hi in cases])
    for k, (label, x, w_lo, w_hi) in enumerate(cases):
        d_lo, d_hi, sens = ps.psens_one(x, w_lo, w_hi)
        cjs_lo, cjs_hi, s = got[3 * k:3 * k + 3]
        assert abs(cjs_lo ** 2 - d_lo) <= x.size * EPS and abs(cjs_hi ** 2 - d_hi) <= x.size * EPS, label
        assert s == (cjs_lo + cjs_hi) / (2.0 * math.log2(1.01)), label
        if label != "uniform":
            assert abs(s - sens) <= 1e-9 * sens, (label, s, sens)
    x = np.arange(6.0)
    x[2] = np.nan
    assert all(math.isnan(v) for v in _run(exe, [[2, 6, 0.01, *x, *np.full(12, 1 / 6)]]))


def test_the_header_reproduces_the_weights(exe):
    worst = 0.0
    for S, kind in ((2, "normal"), (16, "normal"), (25, "normal"), (100, "normal"), (100, "ties"), (1000, "normal")):
        _, lc = synthetic(S, 20 + S, kind)
        if kind == "ties":
            lc = np.round(lc)
        for alpha in ps.alphas():
            got = _run(exe, [[3, S, alpha, *lc]])
            w, khat = ps.weights(lc, alpha)
            assert (got[0] == khat == math.inf) or abs(got[0] - khat) <= 1e-9, (S, kind, alpha, got[0], khat)
            np.testing.assert_allclose(got[1:], w, rtol=1e-9, atol=1e-9 / S)
            assert abs(sum(got[1:]) - 1.0) <= S * EPS
            worst = max(worst, float(np.max(np.abs(np.array(got[1:]) / w - 1.0))))
    print("header: worst relative weight difference", worst)
    lc = np.arange(10.0)
    lc[3] = -np.inf
    assert all(math.isnan(v) for v in _run(exe, [[3, 10, 1.01, *lc]]))


def test_the_program_refuses_malformed_input(exe):
    assert subprocess.run([exe], input="1 3 0x1p0\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="7 4\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="1 1 0.5 1.0\n", capture_output=True, text=True).returncode == 2


# ---- which factor is a variable's prior; the refusals ------------------------------------------------------------------------------------
def test_prior_factors_are_identified():
    spec = pm_.every_family()
    pf = sensitivity.prior_factors(spec)
    assert [n for n, _ in pf] == [v.name for v in spec.vars]
    for name, fi in pf:
        f = spec.factors[fi]
        assert f.name == name and not f.observed
    assert sensitivity.prior_refusal(spec) is None and sensitivity.likelihood_refusal(spec) is None
    assert [n for n, _ in sensitivity.prior_factors(spec, ["sc", "s"])] == ["s", "sc"]
    with pytest.raises(KeyError, match="nope"):
        sensitivity.prior_factors(spec, ["nope"])
    # the family restriction of the prior predictive is dropped: a density can be evaluated for these
    assert sensitivity.prior_refusal(pm_._truncated()) is None
    assert sensitivity.prior_refusal(pm_._by_hand(ms.D_BINOMIAL, "binom", 4)()) is None
    assert sensitivity.prior_refusal(models.eight_schools()) is None
    assert sensitivity.prior_refusal(models.hier_logit(G=4, D=2, rows_per_group=5)) is None


@pytest.mark.parametrize("build, text", [
    (pm_._flat, r"variable 1 \('free'\) has no prior factor"),
    (pm_._twice, r"variable 1 \('twice'\) has more than one prior factor"),
    (lambda: models.mvnormal(n=16, seed=5), r"variable 0 \('x'\) is the MvNormal node's"),
    (pm_.dirichlet_mixture, r"variable 0 \('w'\) holds the mixture node's Dirichlet weights"),
    (pm_._potential_reweights, r"Potential factor 1 \('push'\) reads variable 0 \('pushed'\): PyMC leaves Potentials out of compute_log_prior"),
    (pm_._weibull, r"Potential factor 0 \('weib_logp'\) reads variable 0 \('weib'\): PyMC leaves Potentials out"),
    (pm_._by_hand(ms.D_DERIVED, "deriv", 1), r"variable 1 \('deriv'\) has no prior factor"),
])
def test_prior_refusals_by_name(build, text):
    import re

    spec = build()
    why = sensitivity.prior_refusal(spec)
    assert why is not None and re.search(text, why), why
    with pytest.raises(ValueError, match="log-prior refused: "):
        sensitivity.prior_factors(spec)


def test_likelihood_refusals_are_logliks():
    from pymc_amd import loglik

    spec = models.normal_mixture_bayes(N=40, K=3)
    assert loglik.refusal(spec) is not None and sensitivity.likelihood_refusal(spec) == loglik.refusal(spec)
    assert sensitivity.likelihood_refusal(pm_.chain3()) == "the model has no observed variable"
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0)
    m.Normal("y", mu, 1.0, observed=np.zeros(3))
    assert sensitivity.likelihood_refusal(m.build()) is None


def test_refusals_need_no_device():
    import __graft_entry__ as g

    g.build_engine()
    from pymc_amd import _lib

    lib = _lib.load()
    limit = sensitivity.max_draws()
    assert limit == 8192
    x = np.zeros((limit + 1, 2))
    w = np.full(limit + 1, 1.0 / (limit + 1))
    out = np.full((3, 2), 7.0)
    args = lambda S, P, d: (_lib.dptr(x), S, P, _lib.dptr(w), _lib.dptr(w), d, _lib.dptr(out))   # noqa: E731
    assert lib.nuts_psens(*args(limit + 1, 2, 0.01)) == _lib.NUTS_E_ARG and "8192" in _lib.last_error() and "out of scope" in _lib.last_error()
    assert lib.nuts_psens(*args(1, 2, 0.01)) == _lib.NUTS_E_ARG and "at least 2 draws" in _lib.last_error()
    assert lib.nuts_psens(*args(10, 0, 0.01)) == _lib.NUTS_E_ARG and "at least 1 parameter" in _lib.last_error()
    for d in (0.0, -0.5, math.nan, math.inf):
        assert lib.nuts_psens(*args(10, 2, d)) == _lib.NUTS_E_ARG and "delta" in _lib.last_error()
    import ctypes as C

    khat = C.c_double(7.0)
    for S, alpha in ((1, 1.01), (limit + 1, 1.01), (10, 0.0), (10, math.nan)):
        assert lib.nuts_psens_weights(_lib.dptr(w), S, alpha, _lib.dptr(x), C.byref(khat)) == _lib.NUTS_E_ARG, (S, alpha)
    assert np.all(out == 7.0) and khat.value == 7.0 and np.all(x == 0.0)
    with pytest.raises(ValueError, match="8192.*out of scope"):
        sensitivity.psens_from_arrays(np.zeros((limit + 1, 2)), np.zeros(limit + 1))
    with pytest.raises(ValueError, match="at least 2 draws"):
        sensitivity.psens_from_arrays(np.zeros((1, 2)), np.zeros(1))
    with pytest.raises(ValueError, match="delta"):
        sensitivity.psens_from_arrays(np.zeros((5, 2)), np.zeros(5), delta=0.0)
    from pymc_amd.sampling import sample

    with pytest.raises(ValueError, match="psens=True refused: 2 chains x 5000 draws = 10000 draws per parameter exceed the limit of 8192"):
        sample(draws=5000, tune=10, chains=2, model=models.eight_schools(), psens=True)      # before any sampling
    with pytest.raises(ValueError, match="component"):
        sensitivity.psens(models.eight_schools(), np.zeros((1, 4, 10)), component="posterior")
