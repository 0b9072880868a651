"""Prior draws on the device (csrc/prior.h, csrc/prior_kernel.h, `nuts_model_prior`, pymc_amd/predictive.py) against the NumPy
restatement (tests/prior_reference.py), level by level: the restatement draws each level given the DEVICE's values of the earlier
ones, so one gamma attempt decided the other way does not compound.

Bars: rtol = atol = 1e-10 on every element whose acceptance margin in the restatement exceeds 1e-9, at most 1 element in 1 000 left
out (the count is printed; NaN and infinities must sit where the restatement has them).  Everything about batches, splits and the
existing posterior-predictive path is `array_equal`.  Conditional uniformity and `prior_ppc` as in tests/test_prior_host.py and
tests/test_gpu_predictive.py: sup |ECDF - u| <= 1.95 / sqrt(n) at n = 20 000; sums, means and variances 1e-12 relative against NumPy
in extended precision on the returned matrix, counts and extremes exact.
"""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prior_models as pm_  # noqa: E402
import prior_reference as pref  # noqa: E402
from pymc_amd import _lib, models, predictive, trace  # noqa: E402
from pymc_amd.value_grad import DeviceValueGradFunction  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-10, atol=1e-10)
SEED = 0x9E3779B97F4A7C15


def _vg(spec):
    return DeviceValueGradFunction(spec, device=0)


def _hold(label, got, want, margin):
    assert got.shape == want.shape, label
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), label
    keep = fin & (margin > 1e-9)
    left_out = int((fin & ~keep).sum())
    err = float(np.max(np.abs(got[keep] - want[keep]) / np.maximum(1.0, np.abs(want[keep])))) if keep.any() else 0.0
    print(label, "left out (acceptance margin <= 1e-9):", left_out, "of", got.size, "; max relative error", err)
    assert left_out * 1000 <= got.size, label
    np.testing.assert_allclose(got[keep], want[keep], err_msg=label, **TOL)


def _against_restatement(label, spec, S_list, seed=SEED):
    f = _vg(spec)
    try:
        for S in S_list:
            q, bad = f.prior(S, seed=seed, draw0=5)
            want, margin = pref.sample(spec, S, seed, draw0=5, given=q)
            _hold(f"{label} S={S}", q, want, margin)
            assert bad == int((~np.isfinite(q)).sum())
    finally:
        f.close()


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 63, 64, 65, 257])
def test_two_levels_of_every_transform_at_the_workgroups_edges(size):
    _against_restatement(f"sized {size}", pm_.sized(size), (1, 8, 9, 21))


@pytest.mark.parametrize("label, build", [("three deep", pm_.chain3), ("gather", pm_.gathered), ("every family", lambda: pm_.every_family(65)),
                                          ("Dirichlet K=3", lambda: pm_.dirichlet_mixture(3)), ("Dirichlet K=9", lambda: pm_.dirichlet_mixture(9))],
                         ids=["chain", "gather", "families", "dirichlet3", "dirichlet9"])
def test_programs_gathers_families_and_the_dirichlet_weights(label, build):
    _against_restatement(label, build(), (9, 21))


# ---- 2. batch and split --------------------------------------------------------------------------------------------------------------
def test_a_draw_does_not_depend_on_batch_or_split():
    spec = pm_.every_family(65)
    f = _vg(spec)
    try:
        one, _ = f.prior(21, seed=SEED)
        a, _ = f.prior(8, seed=SEED)
        b, _ = f.prior(13, seed=SEED, draw0=8)
        assert np.array_equal(np.concatenate([a, b]), one, equal_nan=True)
        assert not np.array_equal(f.prior(21, seed=SEED + 1)[0], one)
        try:
            for B in range(1, 65):          # every batch size the engine can be given (option NUTS_PRIOR_B)
                _lib.set_engine_option("NUTS_PRIOR_B", B)
                assert np.array_equal(f.prior(21, seed=SEED)[0], one, equal_nan=True), B
        finally:
            _lib.unset_engine_option("NUTS_PRIOR_B")
        big, _ = f.prior(130, seed=SEED)      # three batches of the default size
        assert np.array_equal(big[:21], one, equal_nan=True)
    finally:
        f.close()


# ---- 3. the existing path ------------------------------------------------------------------------------------------------------------
# (normal_mixture_bayes is the CONDITIONAL mixture and softmax_regression's likelihood is a Potential over the coefficients: the prior of
# both is refused by rule, which is what is held for them; the marginal Dirichlet mixture stands in for the node's replicates)
CONSISTENCY = [
    ("eight schools", models.eight_schools, None),
    ("hier_logit", lambda: models.hier_logit(G=6, D=3, rows_per_group=7), None),
    ("glm normal", lambda: models.glm_nuts(N=300, P=5, family="normal"), None),
    ("glm bernoulli", lambda: models.glm_nuts(N=300, P=5, family="bernoulli"), None),
    ("glm poisson", lambda: models.glm_nuts(N=300, P=5, family="poisson"), None),
    ("normal_mixture_bayes", lambda: models.normal_mixture_bayes(N=200, K=3), "is a conditional mixture"),
    ("marginal Dirichlet mixture", lambda: pm_.dirichlet_mixture(3, N=200), None),
    ("softmax_regression", lambda: models.softmax_regression(N=300, lin=True), "reads a linear predictor: it reweights the prior"),
]


@pytest.mark.parametrize("case", range(len(CONSISTENCY)), ids=[c[0] for c in CONSISTENCY])
def test_prior_predictive_is_the_posterior_predictive_path_at_the_prior_draws(case):
    _, build, refused = CONSISTENCY[case]
    spec = build()
    if refused:
        with pytest.raises(ValueError, match="prior predictive refused.*" + re.escape(refused)):
            predictive.sample_prior_predictive(spec, 11, random_seed=SEED, device=0)
        f = _vg(spec)
        try:
            with pytest.raises(ValueError, match=re.escape(pm_.engine_text(refused))):
                f.prior(1)
        finally:
            f.close()
        return
    out = predictive.sample_prior_predictive(spec, 11, random_seed=SEED, device=0)
    assert out["q"].shape == (1, 11, spec.n) and out["n_nonfinite"] == int((~np.isfinite(out["q"])).sum())
    assert "prior_predictive_refused" not in out and out["prior_predictive"]
    again = predictive.sample_posterior_predictive(spec, out["q"], random_seed=SEED, chain_ids=[0], device=0)
    assert list(again) == list(out["prior_predictive"])
    for name, y in out["prior_predictive"].items():
        assert y.shape[:2] == (1, 11) and np.array_equal(y, again[name], equal_nan=True), name
    back = trace.posterior(spec, out["q"])
    assert list(back) == list(out["prior"])
    for name, x in out["prior"].items():
        assert np.array_equal(x, back[name], equal_nan=True), name


def test_prior_holds_the_deterministics_as_the_trace_records_them():
    spec = pm_.with_deterministics()
    out = predictive.sample_prior_predictive(spec, 9, random_seed=SEED, device=0)
    pr = out["prior"]
    assert list(pr) == ["s", "x", "s2", "ex"] and pr["s2"].shape == (1, 9) and pr["ex"].shape == (1, 9, 6)
    assert np.array_equal(pr["s"], np.exp(out["q"][..., 0]))
    np.testing.assert_allclose(pr["s2"], pr["s"] ** 2, rtol=1e-14)
    np.testing.assert_allclose(pr["ex"], np.exp(pr["x"]) * pr["s"][..., None], rtol=1e-14)
    only = predictive.sample_prior_predictive(spec, 9, var_names=["s2", "y"], random_seed=SEED, device=0)
    assert list(only["prior"]) == ["s2"] and list(only["prior_predictive"]) == ["y"] and np.array_equal(only["prior"]["s2"], pr["s2"])


def test_a_refused_likelihood_still_gets_the_prior():
    from pymc_amd.model_spec import ModelBuilder

    m = ModelBuilder()
    p = m.Beta("p", 2.0, 2.0)
    m.Binomial("k", 10.0, p, observed=np.array([3.0, 5.0]))
    out = predictive.sample_prior_predictive(m.build(), 9, random_seed=1, device=0)
    assert "Binomial" in out["prior_predictive_refused"] and out["prior_predictive"] == {} and out["prior"]["p"].shape == (1, 9)


# ---- 4. conditional uniformity of the device's draws ---------------------------------------------------------------------------------
def test_the_devices_draws_are_uniform_under_their_conditional_cdfs():
    spec = pm_.every_family(250)
    f = _vg(spec)
    try:
        q, bad = f.prior(80, seed=0)
    finally:
        f.close()
    assert bad == 0
    u = pm_.conditional_u(spec, q)
    for name, uu in u.items():
        d = pm_.sup_uniform(uu)
        print(name, "n =", uu.size, "sup |ECDF - u| sqrt(n) =", d * math.sqrt(uu.size))
        assert d <= 1.95 / math.sqrt(uu.size), name
    for child, parent in pm_.parents_elementwise(spec):
        a, b = np.ravel(u[child]), np.ravel(u[parent])
        assert abs(float(np.corrcoef(a, b)[0, 1])) <= 3.29 / math.sqrt(a.size), (child, parent)


# ---- 5. prior_ppc --------------------------------------------------------------------------------------------------------------------
def test_prior_ppc_is_the_summary_of_the_replicates():
    spec = pm_.every_family(65)
    S = 37
    out = predictive.sample_prior_predictive(spec, S, random_seed=SEED, device=0)
    yrep = out["prior_predictive"]["y"][0]
    y = np.linspace(-2.0, 2.0, 65)
    assert yrep.shape == (S, 65) and np.all(np.isfinite(yrep))
    L = yrep.astype(np.longdouble)
    for batch in (64, 5):
        got = predictive.prior_ppc(spec, S, var_name="y", random_seed=SEED, pointwise=True, device=0, batch=batch)
        assert got["n_samples"] == S and got["n_data_points"] == 65
        mean_i = L.mean(axis=0)
        np.testing.assert_allclose(got["mean_i"], mean_i.astype("float64"), rtol=1e-12, atol=0)
        np.testing.assert_allclose(got["var_i"], (((L - mean_i) ** 2).sum(axis=0) / S).astype("float64"), rtol=1e-12, atol=0)
        assert np.array_equal(got["p_i"], ((yrep < y).sum(0) + 0.5 * (yrep == y).sum(0)) / S)
        mean_s = L.sum(axis=1) / 65
        np.testing.assert_allclose(got["T_mean"], mean_s.astype("float64"), rtol=1e-12, atol=0)
        np.testing.assert_allclose(got["T_sd"], np.sqrt((L * L).sum(axis=1) / 65 - mean_s * mean_s).astype("float64"), rtol=1e-12, atol=0)
        assert np.array_equal(got["T_min"], yrep.min(axis=1)) and np.array_equal(got["T_max"], yrep.max(axis=1))
        assert got["p_mean"] == float(np.mean(got["T_mean"] >= got["T_obs"]["mean"]))


# ---- 6. NaN propagation --------------------------------------------------------------------------------------------------------------
def test_invalid_parameters_give_nan_there_and_below_and_only_there():
    spec = pm_.nan_model(9)
    f = _vg(spec)
    try:
        q, bad = f.prior(40, seed=3)
    finally:
        f.close()
    m, x, z = q[:, 0], q[:, 1:10], q[:, 10:19]
    dead = ~(m > 0)
    assert np.all(np.isfinite(m)) and 5 <= dead.sum() <= 35
    assert np.all(np.isnan(x[dead])) and np.all(np.isnan(z[dead])) and np.all(np.isfinite(x[~dead])) and np.all(np.isfinite(z[~dead]))
    assert bad == int((~np.isfinite(q)).sum()) == 18 * int(dead.sum())
    want, margin = pref.sample(spec, 40, 3, given=q)
    _hold("nan model", q, want, margin)


# ---- 7. refusals and the public interface ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [k for k, c in enumerate(pm_.REFUSALS) if c[3]], ids=[c[0] for c in pm_.REFUSALS if c[3]])
def test_the_engine_refuses_by_name_what_the_host_layer_refuses(case):
    _, build, text, _ = pm_.REFUSALS[case]
    spec = build()
    assert text in predictive.prior_refusal(spec)
    f = _vg(spec)
    try:
        with pytest.raises(ValueError, match="prior predictive: .*" + re.escape(pm_.engine_text(text))):
            f.prior(2)
    finally:
        f.close()


def test_the_engine_refuses_draw_numbers_beyond_32_bits_and_a_chain_group_member():
    from pymc_amd.chain_group import ChainGroup
    from pymc_amd.sampling import init_nuts

    f = _vg(models.eight_schools())
    try:
        with pytest.raises(ValueError, match="below 2\\^32"):
            f.prior(2, draw0=2 ** 32 - 1)
        assert f.prior(1, draw0=2 ** 32 - 1)[0].shape == (1, 10)
        assert f.prior(0)[0].shape == (0, 10)
    finally:
        f.close()
    spec = models.mvnormal(n=256, seed=5)
    step = init_nuts(spec, init="adapt_diag", chains=1, random_seed_list=[1], device=0, tune=10)[1]
    group = ChainGroup([step])
    try:
        with pytest.raises(ValueError, match="chain group"):
            step._logp_dlogp_func.prior(1)
    finally:
        group.close()
        step.close()


def test_sample_returns_the_prior_groups_on_request():
    from pymc_amd.sampling import sample

    spec = models.eight_schools()
    res = sample(draws=10, tune=10, chains=1, model=spec, random_seed=19, device=0, prior_predictive=12)
    try:
        assert set(res["prior"]) == {"eta", "mu", "tau"} and res["prior"]["eta"].shape == (1, 12, 8) and np.all(res["prior"]["tau"] > 0)
        assert list(res["prior_predictive"]) == ["obs"] and res["prior_predictive"]["obs"].shape == (1, 12, 8)
        again = predictive.sample_prior_predictive(spec, 12, random_seed=predictive.seed_from(19), device=0)
        assert np.array_equal(again["prior_predictive"]["obs"], res["prior_predictive"]["obs"])
    finally:
        res["step"].close()
    res = sample(draws=3, tune=3, chains=1, model=spec, random_seed=19, device=0)
    assert "prior" not in res and "prior_predictive" not in res
    res["step"].close()
    with pytest.raises(ValueError, match="prior_predictive=True refused: .*MvNormal"):
        sample(draws=3, tune=3, chains=1, model=models.mvnormal(n=16, seed=5), random_seed=1, device=0, prior_predictive=True)
