"""Posterior-predictive variates on the host: the NumPy restatement (tests/predictive_reference.py) reproduces Philox's known
answers and draws from the distributions it claims to (held to `scipy.stats`), and pymc_amd/csrc/predictive.h -- the header
k_pp_draw / k_pp_factor / k_pp_mix compile -- reproduces the restatement.

`tests/predictive_check.cpp` is a stand-alone program around the header (system compiler, -Wall -Wextra -Werror, address and
undefined-behaviour sanitizers when they link); it is never loaded into Python.

Bars.  Distribution: sup |ECDF - CDF| <= 1.95 / sqrt(n), the asymptotic 0.001 level of the Kolmogorov statistic (at the integers
for the discrete families, where the bound is conservative), n = 20 000, seed = the case's number, fixed in advance.  Header against
restatement: continuous values rtol = atol = 1e-10 (the project's bar for device values); discrete values `array_equal` on every
element whose decision margin in the restatement exceeds 1e-9, at most 1 element in 1 000 left out.
"""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predictive_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "predictive_check.cpp")
INC = os.path.join(ROOT, "pymc_amd", "csrc")

N = 20000
KS = 1.95 / math.sqrt(N)
KIND, INDEX = 0, 5

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]

# (label, dist, a1, a2, a3, scipy distribution, discrete)
CASES = [
    ("normal", ref.D_NORMAL, 1.5, 2.0, 0.0, stats.norm(1.5, 2.0), False),
    ("halfnormal", ref.D_HALFNORMAL, 1.3, 0.0, 0.0, stats.halfnorm(scale=1.3), False),
    ("lognormal", ref.D_LOGNORMAL, 0.2, 0.7, 0.0, stats.lognorm(0.7, scale=math.exp(0.2)), False),
    ("cauchy", ref.D_CAUCHY, -1.0, 2.0, 0.0, stats.cauchy(-1.0, 2.0), False),
    ("halfcauchy", ref.D_HALFCAUCHY, 1.5, 0.0, 0.0, stats.halfcauchy(scale=1.5), False),
    ("laplace", ref.D_LAPLACE, 0.5, 1.2, 0.0, stats.laplace(0.5, 1.2), False),
    ("exponential", ref.D_EXPONENTIAL, 2.5, 0.0, 0.0, stats.expon(scale=1 / 2.5), False),
    ("uniform", ref.D_UNIFORM, -1.0, 3.0, 0.0, stats.uniform(-1.0, 4.0), False),
    ("bernoulli", ref.D_BERNOULLI, 0.3, 0.0, 0.0, stats.bernoulli(0.3), True),
    ("bernoulli-logit", ref.D_BERNOULLI_LOGIT, 0.8, 0.0, 0.0, stats.bernoulli(1.0 / (1.0 + math.exp(-0.8))), True),
    ("gamma 0.5", ref.D_GAMMA, 0.5, 2.0, 0.0, stats.gamma(0.5, scale=0.5), False),
    ("gamma 1", ref.D_GAMMA, 1.0, 2.0, 0.0, stats.gamma(1.0, scale=0.5), False),
    ("gamma 2.5", ref.D_GAMMA, 2.5, 2.0, 0.0, stats.gamma(2.5, scale=0.5), False),
    ("gamma 20", ref.D_GAMMA, 20.0, 2.0, 0.0, stats.gamma(20.0, scale=0.5), False),
    ("invgamma", ref.D_INVGAMMA, 3.0, 2.0, 0.0, stats.invgamma(3.0, scale=2.0), False),
    ("beta 0.7 2.5", ref.D_BETA, 0.7, 2.5, 0.0, stats.beta(0.7, 2.5), False),
    ("beta 3 1.5", ref.D_BETA, 3.0, 1.5, 0.0, stats.beta(3.0, 1.5), False),
    ("studentt 4", ref.D_STUDENTT, 4.0, 1.0, 2.0, stats.t(4.0, 1.0, 2.0), False),
    ("studentt 0.8", ref.D_STUDENTT, 0.8, -0.5, 0.7, stats.t(0.8, -0.5, 0.7), False),
    ("poisson 0.3", ref.D_POISSON, 0.3, 0.0, 0.0, stats.poisson(0.3), True),
    ("poisson 4", ref.D_POISSON, 4.0, 0.0, 0.0, stats.poisson(4.0), True),
    ("poisson 9.99", ref.D_POISSON, 9.99, 0.0, 0.0, stats.poisson(9.99), True),
    ("poisson 10", ref.D_POISSON, 10.0, 0.0, 0.0, stats.poisson(10.0), True),
    ("poisson 50", ref.D_POISSON, 50.0, 0.0, 0.0, stats.poisson(50.0), True),
    ("poisson 148", ref.D_POISSON, 148.0, 0.0, 0.0, stats.poisson(148.0), True),
]
IDS = [c[0] for c in CASES]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = ref.philox([np.uint32(c) for c in ctr], key)
        assert " ".join(f"{int(w):08x}" for w in got) == want


def test_uniforms_are_positive_so_their_logarithm_is_finite():
    """k + 0.5 of the 53-bit integer k is exact below 2^52 and rounds to even above: the one value k = 2^53 - 1 gives u = 1.0
    (log u = 0), every other u < 1; the smallest is 2^-54."""
    lo = np.array([0, 0xFFFFFFFF, 0xFFFFFFBF], dtype=np.uint32)
    hi = np.array([0, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
    u = ref.u53(lo, hi)
    assert u[0] == 2.0 ** -54 and u[1] == 1.0 and u[2] == 1.0 - 2.0 ** -52
    assert np.all(np.isfinite(np.log(u)))


def _sup(x, dist, discrete):
    x = np.sort(x)
    n = x.size
    if discrete:
        ks = np.arange(0, int(x.max()) + 2)
        ecdf = np.searchsorted(x, ks, side="right") / n
        return float(np.abs(ecdf - dist.cdf(ks)).max())
    F = dist.cdf(x)
    return float(max((np.arange(1, n + 1) / n - F).max(), (F - np.arange(n) / n).max()))


@pytest.mark.parametrize("axis", ["observations", "draws"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_the_restatement_draws_from_the_family(case, axis):
    label, dist, a1, a2, a3, sp, discrete = CASES[case]
    adr = ref.Address(case, KIND, INDEX, 3, np.arange(N)) if axis == "observations" else ref.Address(case, KIND, INDEX, np.arange(N), 7)
    x, _ = ref.draw(dist, a1, a2, a3, adr)
    assert np.all(np.isfinite(x))
    d = _sup(x, sp, discrete)
    print(label, axis, "sup |ECDF - CDF| sqrt(n) =", d * math.sqrt(N))
    assert d <= KS


def test_the_restatement_of_the_mixture_draws_from_it():
    mu, sg, w = np.array([-2.0, 0.5, 3.0]), np.array([0.5, 1.0, 0.7]), np.array([0.2, 0.5, 0.3])
    x, _ = ref.mixture(mu, sg, w, ref.Address(100, 2, 0, 1, np.arange(N)))

    class Mix:
        @staticmethod
        def cdf(v):
            return sum(wk * stats.norm(m, s).cdf(v) for m, s, wk in zip(mu, sg, w))

    d = _sup(x, Mix, False)
    print("mixture sup |ECDF - CDF| sqrt(n) =", d * math.sqrt(N))
    assert d <= KS


def test_streams_of_two_seeds_nodes_draws_and_observations_differ():
    i = np.arange(1000)
    base = ref.Address(1, 0, 0, 0, i).block(0)[0]
    for other in (ref.Address(2, 0, 0, 0, i), ref.Address(1, 1, 0, 0, i), ref.Address(1, 0, 1, 0, i), ref.Address(1, 0, 0, 1, i),
                  ref.Address(1, 0, 0, 0, i + (1 << 32)), ref.Address(1 + (1 << 32), 0, 0, 0, i)):
        assert not np.any(other.block(0)[0] == base)
    assert not np.any(ref.Address(1, 0, 0, 0, i).block(1)[0] == base)


# ---- the header ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(INC, "predictive.h")), "pymc_amd/csrc/predictive.h is missing"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    out = str(tmp_path_factory.mktemp("predictive") / "predictive_check")
    base = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + INC, SRC, "-o", out]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return out


def _floats(text):
    return np.array([float("nan") if w in ("nan", "-nan") else float.fromhex(w) if "x" in w else float(w) for w in text.split()])


def _run(exe, req, code=0):
    r = subprocess.run([exe], input=req, capture_output=True, text=True)
    assert r.returncode == code, (r.returncode, r.stderr)
    return r.stdout


def _tok(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("inf" if v == math.inf else ("-inf" if v == -math.inf else v.hex()))


def _draw_req(dist, a1, a2, a3, seed, kind, index, s0, ns, i0, ni):
    return f"draw {dist} {_tok(a1)} {_tok(a2)} {_tok(a3)} {seed} {kind} {index} {s0} {ns} {i0} {ni}\n"


def test_the_header_reproduces_the_known_answers(exe):
    for ctr, key, want in KAT:
        assert _run(exe, "philox " + " ".join(hex(v) for v in ctr + key) + "\n").strip() == want


def _hold(label, got, want, margin, discrete):
    assert got.shape == want.shape
    if not discrete:
        assert np.all(np.isfinite(want))
        print(label, "max relative difference", float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))))
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10, err_msg=label)
        return
    keep = margin > 1e-9
    left_out = int((~keep).sum())
    print(label, "elements left out (decision margin <= 1e-9):", left_out, "of", got.size)
    assert left_out * 1000 <= got.size
    assert np.array_equal(got[keep], want[keep]), label


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_the_header_reproduces_the_restatement(exe, case):
    label, dist, a1, a2, a3, _, discrete = CASES[case]
    got = _floats(_run(exe, _draw_req(dist, a1, a2, a3, case, KIND, INDEX, 3, 1, 0, N)))
    want, margin = ref.draw(dist, a1, a2, a3, ref.Address(case, KIND, INDEX, 3, np.arange(N)))
    _hold(label, got, want, margin, discrete)


def test_the_header_addresses_draws_and_wide_indices_as_the_restatement(exe):
    """a [draws x observations] block, draw-major; an observation index past 2^32; the last draw number that fits; a wide seed"""
    seed = 0xFEDCBA9876543210
    for dist, a1, a2, s0, ns, i0, ni in ((ref.D_NORMAL, 0.0, 1.0, 17, 5, 0, 33), (ref.D_GAMMA, 0.6, 1.5, 0, 3, (1 << 32) - 5, 10),
                                         (ref.D_EXPONENTIAL, 1.0, 0.0, (1 << 32) - 2, 2, 1 << 40, 4)):
        got = _floats(_run(exe, _draw_req(dist, a1, a2, 0.0, seed, 3, 0x3FFF, s0, ns, i0, ni))).reshape(ns, ni)
        want, _ = ref.draw(dist, a1, a2, 0.0, ref.Address(seed, 3, 0x3FFF, (s0 + np.arange(ns))[:, None], (i0 + np.arange(ni))[None, :]))
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10)


def test_the_header_reproduces_the_mixture(exe):
    rng = np.random.default_rng(5)
    for K in (1, 3, 9):
        mu, sg = rng.normal(size=K) * 2.0, 0.5 + rng.random(K)
        w = rng.dirichlet(np.ones(K))
        req = f"mix {K} " + " ".join(_tok(v) for v in np.concatenate([mu, sg, w])) + f" 9 2 0 4 1 0 {N}\n"
        got = _floats(_run(exe, req))
        want, margin = ref.mixture(mu, sg, w, ref.Address(9, 2, 0, 4, np.arange(N)))
        keep = margin > 1e-9
        print("mixture K", K, "left out", int((~keep).sum()))
        assert (~keep).sum() * 1000 <= N
        np.testing.assert_allclose(got[keep], want[keep], rtol=1e-10, atol=1e-10)


INVALID = [(ref.D_NORMAL, 0.0, -1.0, 0.0), (ref.D_NORMAL, 0.0, 0.0, 0.0), (ref.D_NORMAL, 0.0, math.nan, 0.0), (ref.D_HALFNORMAL, -0.5, 0.0, 0.0),
           (ref.D_CAUCHY, 0.0, 0.0, 0.0), (ref.D_HALFCAUCHY, -1.0, 0.0, 0.0), (ref.D_STUDENTT, 4.0, 0.0, -1.0), (ref.D_EXPONENTIAL, 0.0, 0.0, 0.0),
           (ref.D_UNIFORM, 1.0, 0.5, 0.0), (ref.D_LOGNORMAL, 0.0, -2.0, 0.0), (ref.D_BERNOULLI, 1.5, 0.0, 0.0), (ref.D_BERNOULLI, -0.1, 0.0, 0.0),
           (ref.D_GAMMA, -1.0, 1.0, 0.0), (ref.D_GAMMA, 1.0, -1.0, 0.0), (ref.D_INVGAMMA, 1.0, 0.0, 0.0), (ref.D_LAPLACE, 0.0, -1.0, 0.0),
           (ref.D_POISSON, -0.5, 0.0, 0.0), (ref.D_POISSON, math.nan, 0.0, 0.0), (ref.D_BERNOULLI_LOGIT, math.nan, 0.0, 0.0)]


def test_invalid_parameters_give_nan_in_both(exe):
    req = "".join(_draw_req(d, a1, a2, a3, 1, 0, 0, 0, 2, 0, 3) for d, a1, a2, a3 in INVALID)
    got = _floats(_run(exe, req))
    assert got.size == 6 * len(INVALID) and np.all(np.isnan(got))
    for d, a1, a2, a3 in INVALID:
        assert np.all(np.isnan(ref.draw(d, a1, a2, a3, ref.Address(1, 0, 0, np.arange(2)[:, None], np.arange(3)[None, :]))[0]))
    # the edges that ARE valid: Bernoulli p = 0 / 1, Poisson mu = 0, Uniform of zero width
    edge = _floats(_run(exe, _draw_req(ref.D_BERNOULLI, 0.0, 0, 0, 1, 0, 0, 0, 1, 0, 50) + _draw_req(ref.D_BERNOULLI, 1.0, 0, 0, 1, 0, 0, 0, 1, 0, 50)
                        + _draw_req(ref.D_POISSON, 0.0, 0, 0, 1, 0, 0, 0, 1, 0, 50) + _draw_req(ref.D_UNIFORM, 2.0, 2.0, 0, 1, 0, 0, 0, 1, 0, 50)))
    assert np.array_equal(edge, np.repeat([0.0, 1.0, 0.0, 2.0], 50))


def test_the_program_refuses_what_is_out_of_scope(exe):
    for dist in (ref.D_TRUNCNORMAL, ref.D_POTENTIAL, ref.D_BINOMIAL, ref.D_DERIVED, 19):
        _run(exe, _draw_req(dist, 0.0, 1.0, 0.0, 1, 0, 0, 0, 1, 0, 1), code=4)
        with pytest.raises(ValueError, match="refused"):
            ref.draw(dist, 0.0, 1.0, 0.0, ref.Address(1, 0, 0, 0, np.arange(1)))
    _run(exe, _draw_req(0, 0.0, 1.0, 0.0, 1, 0, 0x4000, 0, 1, 0, 1), code=4)        # the node's index does not fit 14 bits
    _run(exe, _draw_req(0, 0.0, 1.0, 0.0, 1, 4, 0, 0, 1, 0, 1), code=4)             # nor this kind its 2
    _run(exe, _draw_req(0, 0.0, 1.0, 0.0, 1, 0, 0, (1 << 32) - 1, 2, 0, 1), code=4)  # draw numbers past 2^32
    _run(exe, "draw 0 0x1p0 1.0x 0 1 0 0 0 1 0 1\n", code=2)
    _run(exe, "what\n", code=2)


# ---- the Python side: refusals and the host arithmetic of the checks --------------------------------------------------------------
def test_refusal_names_the_family():
    from pymc_amd import models, predictive
    from pymc_amd import model_spec as ms
    from pymc_amd.model_spec import ModelBuilder

    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    m.Normal("y_ok", a, 1.0, observed=np.zeros(3))
    m.Binomial("y_bin", 10.0, m.math.sigmoid(a), observed=np.ones(4))
    spec = m.build()
    nodes = {nd[0]: nd for nd in ms.observed_nodes(spec)}
    assert predictive.refusal(spec, [nodes["y_ok"]]) is None
    assert "Binomial" in predictive.refusal(spec, [nodes["y_bin"]]) and "y_bin" in predictive.refusal(spec)
    with pytest.raises(ValueError, match="Binomial"):
        predictive.sample_posterior_predictive(spec, np.zeros((1, 2, spec.n)))
    with pytest.raises(ValueError, match="Binomial"):
        predictive.ppc(spec, np.zeros((1, 2, spec.n)), var_name="y_bin")
    with pytest.raises(KeyError, match="not observed"):
        predictive.sample_posterior_predictive(spec, np.zeros((1, 2, spec.n)), var_names=["a"])
    with pytest.raises(TypeError, match="var_name cannot be None"):
        predictive.ppc(spec, np.zeros((1, 2, spec.n)))
    cond = models.normal_mixture(N=50, K=3, form="node")
    cond.extra = {}
    assert "conditional mixture" in predictive.refusal(cond)
    assert "another step method" in predictive.refusal(models.normal_mixture(N=50, K=3))
    assert predictive.sample_posterior_predictive(models.std_normal(), np.zeros((1, 2, 1))) == {}


def test_sample_refuses_before_sampling():
    from pymc_amd.model_spec import ModelBuilder
    from pymc_amd.sampling import sample

    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    m.Binomial("y_bin", 10.0, m.math.sigmoid(a), observed=np.ones(4))
    with pytest.raises(ValueError, match="posterior_predictive=True refused.*Binomial"):
        sample(draws=5, tune=5, chains=1, model=m.build(), random_seed=1, posterior_predictive=True)


def test_seed_of_sample_is_the_documented_one():
    from pymc_amd import predictive

    assert predictive.seed_from(19) == int(np.random.SeedSequence(19).generate_state(1, np.uint64)[0])


def test_ppc_from_accumulators_is_the_numpy_summary():
    from pymc_amd import predictive

    rng = np.random.default_rng(6)
    S, n = 40, 11
    y = rng.poisson(3.0, n).astype("float64")
    yrep = rng.poisson(3.0, (S, n)).astype("float64")
    T = np.stack([yrep.sum(1), (yrep ** 2).sum(1), yrep.min(1), yrep.max(1)], axis=1)
    T_obs = np.array([y.sum(), (y ** 2).sum(), y.min(), y.max()])
    out = predictive.ppc_from_accumulators(yrep.mean(0), yrep.var(0), (yrep < y).sum(0), (yrep == y).sum(0), T, T_obs, S, pointwise=True)
    np.testing.assert_allclose(out["p_i"], ((yrep < y).sum(0) + 0.5 * (yrep == y).sum(0)) / S)
    np.testing.assert_allclose(out["T_mean"], yrep.mean(1), rtol=1e-13)
    np.testing.assert_allclose(out["T_sd"], yrep.std(1), rtol=1e-9)
    assert np.array_equal(out["T_min"], yrep.min(1)) and np.array_equal(out["T_max"], yrep.max(1))
    assert out["p_mean"] == float(np.mean(yrep.mean(1) >= y.mean())) and out["p_max"] == float(np.mean(yrep.max(1) >= y.max()))
    assert out["p_min"] == float(np.mean(yrep.min(1) >= y.min()))
    assert out["p_sd"] == float(np.mean(out["T_sd"] >= out["T_obs"]["sd"]))
    assert out["n_samples"] == S and out["n_data_points"] == n
    assert "p_i" not in predictive.ppc_from_accumulators(yrep.mean(0), yrep.var(0), (yrep < y).sum(0), (yrep == y).sum(0), T, T_obs, S)
    # NaN replicates are not hidden: a NaN draw makes the p-values NaN, a NaN observation its own p_i
    Tn, mn = T.copy(), yrep.mean(0)
    Tn[3], mn[2] = np.nan, np.nan
    bad = predictive.ppc_from_accumulators(mn, yrep.var(0), (yrep < y).sum(0), (yrep == y).sum(0), Tn, T_obs, S, pointwise=True)
    assert all(np.isnan(bad["p_" + k]) for k in predictive.STATS) and np.array_equal(np.isnan(bad["p_i"]), np.arange(n) == 2)


def test_the_calls_refuse_a_null_handle():
    import ctypes as C

    import __graft_entry__ as g

    g.build_engine()
    from pymc_amd import _lib

    lib = _lib.load()
    out = np.full(4, 7.0)
    n = C.c_int64(-1)
    assert lib.nuts_model_predictive(None, 0, 0, _lib.dptr(out), 1, 0, 0, _lib.dptr(out)) == _lib.NUTS_E_ARG
    assert not lib.nuts_ppc_create(None, 0, 0, 0)
    assert lib.nuts_ppc_update(None, _lib.dptr(out), 1) == _lib.NUTS_E_ARG
    assert lib.nuts_ppc_read(None, None, None, None, None, C.byref(n)) == _lib.NUTS_E_ARG and n.value == -1
    assert lib.nuts_ppc_read_stats(None, _lib.dptr(out), _lib.dptr(out)) == _lib.NUTS_E_ARG
    lib.nuts_ppc_destroy(None)
    assert np.all(out == 7.0)
