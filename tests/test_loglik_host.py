"""Host side of the pointwise log-likelihood (pymc_amd/loglik.py, model_spec.observed_nodes): runs without a GPU."""

import ctypes as C
import os
import sys

import numpy as np
import pytest
from scipy.special import logsumexp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pymc_amd import loglik, models  # noqa: E402
from pymc_amd import model_spec as ms  # noqa: E402
from pymc_amd.model_spec import ModelBuilder  # noqa: E402


def test_observed_nodes_of_builder_specs():
    spec = models.eight_schools()
    assert ms.observed_nodes(spec) == [("obs", ms.LL_FACTOR, 3, 8)]
    assert [f.observed for f in spec.factors] == [False, False, False, True]
    assert ms.observed_nodes(models.std_normal()) == []
    assert ms.observed_nodes(models.mvnormal(n=16)) == []          # a prior, not observed
    spec = models.hier_logit(G=4, D=3, rows_per_group=5)
    assert ms.observed_nodes(spec) == [("y", ms.LL_LOGIT_ROWS, 0, 20)]
    spec = models.glm_nuts(N=30, P=9, family="normal")               # sigma's prior etc. are not observed; the node is
    assert ms.observed_nodes(spec) == [("y", ms.LL_GLM, 0, 30)]
    spec = models.normal_mixture_bayes(N=40)
    assert ms.observed_nodes(spec) == [("y", ms.LL_MIXTURE, 0, 40)]
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    m.Potential("pot", a * a)
    m.Poisson("counts", m.math.exp(a), observed=np.array([1.0, 0.0, 3.0]))
    assert ms.observed_nodes(m.build()) == [("counts", ms.LL_FACTOR, 2, 3)]


def test_a_derived_beta_is_not_an_observed_factor():
    rng = np.random.default_rng(0)
    m = ModelBuilder()
    mu, tau, z = m.Normal("mu", 0.0, 1.0), m.HalfNormal("tau", 1.0), m.Normal("z", 0.0, 1.0, shape=4)
    m.GLM("y", rng.normal(size=(10, 4)), mu + tau * z, rng.normal(size=10))
    spec = m.build()
    assert any(f.dist == ms.D_DERIVED for f in spec.factors)
    assert ms.observed_nodes(spec) == [("y", ms.LL_GLM, 0, 10)]


def _stub(name, fixture=None):
    import lowering_models as lm
    import stubgraph as sg

    return sg.FrozenModel(sg.load_models(fixture or lm.FIXTURE)[name])


def test_observed_nodes_of_a_lowered_graph_with_and_without_logp_observed():
    import more_models as tm
    from pymc_amd.lowering import lower_to_spec

    model = _stub("stochastic_volatility", tm.FIXTURE)
    plain = lower_to_spec(model)
    assert ms.observed_nodes(plain) == [] and not any(f.observed for f in plain.factors)       # absent: all False
    model.logp_observed = [nm == "returns" for nm in model.logp_names]
    spec = lower_to_spec(model)
    assert ms.observed_nodes(spec) == [("returns", ms.LL_FACTOR, next(i for i, f in enumerate(spec.factors) if f.name == "returns"), tm.T_SV)]
    # marking changes nothing else of the spec
    assert [(f.name, f.dist, f.size, f.args, f.prog) for f in spec.factors] == [(f.name, f.dist, f.size, f.args, f.prog) for f in plain.factors]


def test_rows_order_round_trip():
    rng = np.random.default_rng(1)
    G, D, N = 5, 3, 40
    gidx = rng.integers(0, G, size=N).astype("int32")
    X, y = rng.normal(size=(N, D)), (rng.random(N) < 0.5).astype("int8")

    def build(X, y, g):
        m = ModelBuilder()
        mu, sg, z = m.Normal("mu", 0.0, 1.0, shape=D), m.HalfNormal("sigma", 1.0, shape=D), m.Normal("z", 0.0, 1.0, shape=(G, D))
        m.HierLogitRows("y", X, y, g, mu, sg, z)
        return m.build()

    spec = build(X, y, gidx)
    order = spec.rows_order
    assert order is not None and sorted(order) == list(range(N))
    assert np.array_equal(spec.logit_rows.X, X[order]) and np.array_equal(spec.logit_rows.group_idx, gidx[order])
    sorted_values = np.arange(N, dtype="float64")[order] * 2.0             # a value per SORTED row that names the caller's row
    back = loglik.caller_order(spec, ms.LL_LOGIT_ROWS, np.stack([sorted_values, sorted_values + 1.0]))
    assert np.array_equal(back, np.stack([np.arange(N) * 2.0, np.arange(N) * 2.0 + 1.0]))
    # rows passed sorted: no permutation is kept and nothing moves
    o = np.argsort(gidx, kind="stable")
    spec2 = build(X[o], y[o], gidx[o])
    assert spec2.rows_order is None
    assert loglik.caller_order(spec2, ms.LL_LOGIT_ROWS, sorted_values) is sorted_values
    assert loglik.caller_order(spec, ms.LL_GLM, sorted_values) is sorted_values


def test_waic_finalisation_against_two_pass_numpy():
    rng = np.random.default_rng(2)
    S, N = 53, 17
    ll = rng.normal(size=(S, N)) * 2.0 - 3.0
    ll[:, 3] *= 0.01
    # the accumulators as the device forms them: running maximum / rescaled sum, Welford in draw order
    m = np.full(N, -np.inf)
    r, mean, m2 = np.zeros(N), np.zeros(N), np.zeros(N)
    for s in range(S):
        v = ll[s]
        up = v > m
        r = np.where(up, np.where(np.isneginf(m), 0.0, r * np.exp(np.where(up, m - v, 0.0))) + 1.0, r + np.exp(np.where(up, 0.0, v - m)))
        m = np.where(up, v, m)
        d = v - mean
        mean = mean + d / (s + 1)
        m2 = m2 + d * (v - mean)
    out = loglik.waic_from_accumulators(m, r, mean, m2, S, pointwise=True)
    lppd_i = logsumexp(ll, axis=0) - np.log(S)
    p_i = np.var(ll, axis=0)
    elpd_i = lppd_i - p_i
    np.testing.assert_allclose(out["lppd_i"], lppd_i, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out["p_waic_i"], p_i, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(out["waic_i"], elpd_i, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(out["elpd_waic"], elpd_i.sum(), rtol=1e-12)
    np.testing.assert_allclose(out["p_waic"], p_i.sum(), rtol=1e-12)
    np.testing.assert_allclose(out["lppd"], lppd_i.sum(), rtol=1e-12)
    np.testing.assert_allclose(out["se"], np.sqrt(N * np.var(elpd_i)), rtol=1e-12)
    assert out["n_samples"] == S and out["n_data_points"] == N and out["warning"] is True
    assert set(loglik.waic_from_accumulators(m, r, mean, m2, S)) == {"elpd_waic", "se", "p_waic", "lppd", "n_samples", "n_data_points", "warning"}
    calm = loglik.waic_from_accumulators(m, r, mean, m2 * 1e-3, S)
    assert calm["warning"] is False


def test_to_inference_dict_log_likelihood_group():
    from pymc_amd.backends import multitrace_from_result, to_inference_dict

    spec = models.eight_schools()
    rng = np.random.default_rng(3)
    chains, draws = 2, 6
    stats = [[{"depth": int(rng.integers(1, 6)), "energy": float(rng.normal()), "diverging": False, "warning": None} for _ in range(draws)]
             for _ in range(chains)]
    result = {"draws": rng.normal(size=(chains, draws, spec.n)), "stats": stats}
    trace = multitrace_from_result(spec, result)
    base = to_inference_dict(trace)
    assert "log_likelihood" not in base                                        # the default: exactly what it returned before
    ll = {"obs": rng.normal(size=(chains, draws, 8))}
    out = to_inference_dict(trace, log_likelihood=ll)
    assert set(out) == set(base) | {"log_likelihood"}
    assert out["log_likelihood"]["obs"].shape == (chains, draws, 8) and np.array_equal(out["log_likelihood"]["obs"], ll["obs"])
    for grp in ("posterior", "sample_stats"):
        assert set(out[grp]) == set(base[grp]) and all(np.array_equal(out[grp][k], base[grp][k]) for k in base[grp])
    with pytest.raises(ValueError, match="chain, draw"):
        to_inference_dict(trace, log_likelihood={"obs": np.zeros((chains, draws + 1, 8))})


def test_refusals_carry_their_reason():
    # a spec with extra inputs: another step method's state per draw
    spec = models.normal_mixture(N=50, K=3)
    assert spec.extra
    with pytest.raises(ValueError, match="extra inputs.*another step method"):
        loglik.compute_log_likelihood(spec, np.zeros((1, 2, spec.n)))
    with pytest.raises(ValueError, match="another step method"):
        loglik.waic(spec, np.zeros((1, 2, spec.n)), var_name="y|c")
    # the conditional mixture itself (the refusal does not rest on `extra` alone)
    cond = models.normal_mixture(N=50, K=3, form="node")
    cond.extra = {}
    with pytest.raises(ValueError, match="conditional mixture"):
        loglik.compute_log_likelihood(cond, np.zeros((1, 2, cond.n)))
    from pymc_amd.sampling import sample

    with pytest.raises(ValueError, match="log_likelihood=True refused"):
        sample(draws=2, tune=2, chains=1, model=models.normal_mixture(N=50, K=3), log_likelihood=True)
    # several observed variables: `var_name` is required, as in ArviZ
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    m.Normal("y1", a, 1.0, observed=np.zeros(3))
    m.Normal("y2", a, 2.0, observed=np.ones(4))
    two = m.build()
    with pytest.raises(TypeError, match="var_name cannot be None"):
        loglik.waic(two, np.zeros((1, 2, two.n)))
    with pytest.raises(KeyError, match="not observed"):
        loglik.compute_log_likelihood(two, np.zeros((1, 2, two.n)), var_names=["a"])
    with pytest.raises(ValueError, match="raveled unconstrained"):
        loglik._draws_array(np.zeros((1, 2, two.n + 1)), two.n)


def test_a_model_without_observed_variables_gives_an_empty_dict():
    spec = models.std_normal()
    assert loglik.compute_log_likelihood(spec, np.zeros((1, 3, spec.n))) == {}      # (no device is asked)


def test_new_calls_fail_loudly_without_a_device():
    """As `test_no_cpu_fallback` for the old calls: no model can exist without a GPU, and the new entry points refuse a null handle
    instead of computing anything on the host."""
    import __graft_entry__ as g

    g.build_engine()
    from pymc_amd import _lib

    lib = _lib.load()
    n = C.c_int64(-1)
    out = np.full(4, 7.0)
    assert lib.nuts_model_loglik_size(None, 0, 0, C.byref(n)) == _lib.NUTS_E_ARG and n.value == -1
    assert lib.nuts_model_loglik(None, 0, 0, _lib.dptr(out), 1, _lib.dptr(out)) == _lib.NUTS_E_ARG
    assert not lib.nuts_waic_create(None, 0, 0)
    assert lib.nuts_waic_update(None, _lib.dptr(out), 1) == _lib.NUTS_E_ARG
    assert lib.nuts_waic_read(None, None, None, None) == _lib.NUTS_E_ARG
    assert lib.nuts_waic_read_raw(None, _lib.dptr(out)) == _lib.NUTS_E_ARG
    lib.nuts_waic_destroy(None)
    assert np.all(out == 7.0)
    if lib.nuts_device_count() > 0:
        return      # (a GPU is visible: the loud failure of model creation is for GPU-less hosts)
    spec = models.eight_schools()
    with pytest.raises(_lib.EngineError, match="no HIP device|no CPU fallback"):
        loglik.compute_log_likelihood(spec, np.zeros((1, 2, spec.n)))
    with pytest.raises(_lib.EngineError, match="no HIP device|no CPU fallback"):
        loglik.waic(spec, np.zeros((1, 2, spec.n)))
