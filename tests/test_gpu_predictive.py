"""Posterior predictive on the device (csrc/predictive.h, csrc/predictive_kernel.h, pymc_amd/predictive.py) against the NumPy
restatement of the variates (tests/predictive_reference.py), and the streaming predictive checks.

The models and draw scales are those of tests/test_gpu_loglik.py (seeded unconstrained draws ~ N(0, 0.5^2), covariates scaled so that
|eta| <= 5).  The restatement is fed each node's parameters at each draw from the NumPy restatements of the nodes there (the
oracle's forward sweep for the factors) and the address (seed, node, global draw index, observation index in the node's
evaluation order).  Bars: continuous replicates rtol = atol = 1e-10 (the project's bar for device values); discrete replicates
`array_equal` on every element whose decision margin in the restatement exceeds 1e-9, at most 1 element in 1 000 left out (and, for
the mixture, the elements whose component pick has such a margin).  Everything about batches, splits, layouts and seeds is
`array_equal`.  Accumulators against NumPy on the matrix `nuts_model_predictive` returned: counts and min / max exact; means,
variances and sums 1e-12 relative.
"""

import os
import sys

import numpy as np
import pytest
from scipy.special import logsumexp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import predictive_reference as ref  # noqa: E402
import test_gpu_loglik as tl  # noqa: E402
from oracle import ref_models  # noqa: E402
from pymc_amd import loglik, models, predictive  # noqa: E402
from pymc_amd import model_spec as ms  # noqa: E402
from pymc_amd.model_spec import ModelBuilder  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-10, atol=1e-10)
B = tl.B
SEED = 0x9E3779B97F4A7C15
DISCRETE = (ms.D_BERNOULLI, ms.D_BERNOULLI_LOGIT, ms.D_POISSON)


def _hold(label, got, want, margin, discrete):
    assert got.shape == want.shape, label
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), label
    keep = ~nan & ((margin > 1e-9) if discrete else np.ones(want.shape, dtype=bool))
    left_out = int((~keep & ~nan).sum())
    print(label, "left out (decision margin <= 1e-9):", left_out, "of", got.size)
    assert left_out * 1000 <= got.size, label
    if discrete:
        assert np.array_equal(got[keep], want[keep]), label
    else:
        print(label, "max abs err", float(np.abs(got[keep] - want[keep]).max()) if keep.any() else 0.0)
        np.testing.assert_allclose(got[keep], want[keep], err_msg=label, **TOL)


# ---- references: the nodes' parameters at every draw, then the restatement ------------------------------------------------------
def ref_factor(spec, fi, q, seed, draw0=0):
    f = spec.factors[fi]
    out, margin = np.empty((len(q), f.size)), np.empty((len(q), f.size))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s, qs in enumerate(q):
            x = tl._constrained(spec, qs)
            derived = {i: np.broadcast_to(ref_models._forward(spec, g, x)[0][0], (g.size,)) for i, g in enumerate(spec.factors) if g.dist == ms.D_DERIVED}
            args, _, _, _, dead = ref_models._forward(spec, f, x, derived)
            a = [args[k] if k < len(args) else 0.0 for k in (1, 2, 3)]
            v, mg = ref.draw(f.dist, a[0], a[1], a[2], ref.Address(seed, ms.LL_FACTOR, fi, draw0 + s, np.arange(f.size)))
            out[s], margin[s] = (np.nan if dead else v), mg
    return out, margin


def glm_parameters(spec, q):
    """(eta [S, N], sigma [S]) as tests/test_gpu_loglik.py ref_glm forms them"""
    node = spec.glm_rows
    eta, sigma = np.empty((len(q), node.y.size)), np.ones(len(q))
    for s, qs in enumerate(q):
        x = tl._constrained(spec, qs)
        if node.beta is not None:
            v = spec.vars[node.beta]
            beta = x[v.offset : v.offset + v.size]
        else:
            beta = np.broadcast_to(ref_models._forward(spec, spec.factors[node.beta_derived], x)[0][0], (node.X.shape[1],))
        eta[s] = node.X @ beta + (x[spec.vars[node.intercept].offset] if node.intercept is not None else 0.0)
        if node.family == ms.GLM_NORMAL:
            sigma[s] = x[spec.vars[node.sigma].offset] if node.sigma is not None else node.sigma_const
    assert np.abs(eta).max() <= 5.0
    return eta, sigma


def ref_glm(spec, q, seed, draw0=0):
    eta, sigma = glm_parameters(spec, q)
    S, N = eta.shape
    adr = ref.Address(seed, ms.LL_GLM, 0, (draw0 + np.arange(S))[:, None], np.arange(N)[None, :])
    fam = spec.glm_rows.family
    if fam == ms.GLM_NORMAL:
        return ref.draw(ref.D_NORMAL, eta, sigma[:, None], 0.0, adr) + (False,)
    if fam == ms.GLM_BERNOULLI:
        return ref.draw(ref.D_BERNOULLI_LOGIT, eta, 0.0, 0.0, adr) + (True,)
    return ref.draw(ref.D_POISSON, np.exp(eta), 0.0, 0.0, adr) + (True,)


def ref_rows(spec, q, X, gidx, seed, draw0=0):
    """In the spec's group-SORTED order (the order the node evaluates and addresses its rows in)."""
    node = spec.logit_rows
    vm, vs, vz = (spec.vars[i] for i in (node.mu, node.sigma, node.z))
    D = vm.size
    order = np.asarray(spec.rows_order)
    eta = np.empty((len(q), len(gidx)))
    for s, qs in enumerate(q):
        x = tl._constrained(spec, qs)
        beta = x[vm.offset : vm.offset + D] + x[vs.offset : vs.offset + D] * x[vz.offset : vz.offset + vz.size].reshape(-1, D)
        eta[s] = np.einsum("nd,nd->n", X, beta[gidx])[order]
    assert np.abs(eta).max() <= 5.0
    adr = ref.Address(seed, ms.LL_LOGIT_ROWS, 0, (draw0 + np.arange(len(q)))[:, None], np.arange(len(gidx))[None, :])
    return ref.draw(ref.D_BERNOULLI_LOGIT, eta, 0.0, 0.0, adr)


def ref_mix(spec, q, seed, draw0=0):
    node = spec.mixture_rows
    K, N = node.K, node.y.size
    out, margin = np.empty((len(q), N)), np.empty((len(q), N))
    for s, qs in enumerate(q):
        x = tl._constrained(spec, qs)
        mu = x[spec.vars[node.mu].offset :][:K]
        sigma = x[spec.vars[node.sigma].offset :][:K] if node.sigma is not None else np.broadcast_to(np.asarray(node.sigma_const, dtype="float64"), (K,))
        if node.w_alpha is not None:
            yv = x[spec.vars[node.w_logits].offset :][: K - 1]
            e = np.concatenate([yv, [-yv.sum()]])
            w = np.exp(e - logsumexp(e))
        elif node.w_logits is not None:
            e = x[spec.vars[node.w_logits].offset :][:K]
            w = np.exp(e - logsumexp(e))
        else:
            w = np.asarray(node.w_const, dtype="float64")
        out[s], margin[s] = ref.mixture(mu, sigma, w, ref.Address(seed, ms.LL_MIXTURE, 0, draw0 + s, np.arange(N)))
    return out, margin


# ---- 1. element-wise factors --------------------------------------------------------------------------------------------------
def factor_model(N, seed=1):
    """One observed factor per accepted family, one of them through a gather."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=N)
    idx = rng.integers(0, 5, size=N)
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    b = m.Normal("b", 0.0, 1.0)
    s = m.HalfNormal("s", 1.0)
    g = m.Normal("g", 0.0, 1.0, shape=5)
    lin = a + b * m.as_expr(x)
    pos = rng.gamma(2.0, size=N)
    unit = rng.uniform(0.05, 0.95, size=N)
    m.Normal("y_normal", lin, s, observed=rng.normal(size=N))
    m.HalfNormal("y_halfnormal", s, observed=pos)
    m.Cauchy("y_cauchy", lin, s, observed=rng.normal(size=N))
    m.HalfCauchy("y_halfcauchy", s, observed=pos)
    m.StudentT("y_studentt", 4.0, lin, s, observed=rng.normal(size=N))
    m.Beta("y_beta", 0.7, 2.5, observed=unit)
    m.Exponential("y_exponential", m.math.exp(lin), observed=pos)
    m.Uniform("y_uniform", -1.0, 3.0, observed=unit)
    m.BernoulliLogit("y_bernoulli_logit", lin, observed=(rng.random(N) < 0.5).astype("float64"))
    m.LogNormal("y_lognormal", lin, s, observed=pos)
    m.Bernoulli("y_bernoulli", m.math.sigmoid(lin), observed=(rng.random(N) < 0.5).astype("float64"))
    m.Gamma("y_gamma", 0.6, m.math.exp(lin), observed=pos)
    m.Gamma("y_gamma_big", 7.5, s, observed=pos)
    m.InverseGamma("y_invgamma", 3.0, s, observed=pos)
    m.Laplace("y_laplace", lin, s, observed=rng.normal(size=N))
    m.Poisson("y_poisson", m.math.exp(lin), observed=rng.poisson(1.5, size=N).astype("float64"))
    m.Poisson("y_poisson_big", m.math.exp(3.5 + lin), observed=rng.poisson(30.0, size=N).astype("float64"))
    m.Normal("y_gather", g[idx], 1.0, observed=rng.normal(size=N))
    return m.build()


FAMILIES = {ms.D_NORMAL, ms.D_HALFNORMAL, ms.D_CAUCHY, ms.D_HALFCAUCHY, ms.D_STUDENTT, ms.D_BETA, ms.D_EXPONENTIAL, ms.D_UNIFORM, ms.D_BERNOULLI_LOGIT,
            ms.D_LOGNORMAL, ms.D_BERNOULLI, ms.D_GAMMA, ms.D_INVGAMMA, ms.D_LAPLACE, ms.D_POISSON}


@pytest.mark.parametrize("N", [1, 257])
def test_factors_of_every_family_against_the_restatement(N):
    spec = factor_model(N)
    nodes = ms.observed_nodes(spec)
    assert {spec.factors[nd[2]].dist for nd in nodes} == FAMILIES
    q = tl._draws(spec, 9, seed=N)
    got = predictive.sample_posterior_predictive(spec, q[None], random_seed=SEED, device=0)
    assert list(got) == [nd[0] for nd in nodes]
    for name, kind, index, size in nodes:
        want, margin = ref_factor(spec, index, q, SEED)
        assert size == N and got[name].shape == (1, 9, N) and not np.any(np.isnan(want)), name
        _hold(f"{name} N={N}", got[name][0], want, margin, spec.factors[index].dist in DISCRETE)


def derived_model():
    """A derived vector (the GLM's beta = mu0 + tau z) in the model: its factors go one draw at a time."""
    rng = np.random.default_rng(21)
    X = rng.normal(size=(300, 9)) * 0.05
    m = ModelBuilder()
    alpha = m.Normal("alpha", 0.0, 5.0)
    mu0 = m.Normal("mu0", 0.0, 1.0)
    tau = m.HalfNormal("tau", 1.0)
    z = m.Normal("z", 0.0, 1.0, shape=9)
    m.Gamma("y_side", 2.5, m.math.exp(alpha), observed=rng.gamma(2.5, size=40))
    m.GLM("y", X, mu0 + tau * z, rng.normal(size=300), family="normal", intercept=alpha, sigma=0.8)
    return m.build()


def test_factor_and_glm_of_a_model_with_a_derived_vector():
    spec = derived_model()
    assert spec.glm_rows.beta is None
    q = tl._draws(spec, B + 1, seed=22)
    got = predictive.sample_posterior_predictive(spec, q[None], random_seed=SEED, device=0)
    fi = next(nd[2] for nd in ms.observed_nodes(spec) if nd[0] == "y_side")
    want, margin = ref_factor(spec, fi, q, SEED)
    _hold("y_side", got["y_side"][0], want, margin, False)
    want, margin, discrete = ref_glm(spec, q, SEED)
    _hold("y (derived beta)", got["y"][0], want, margin, discrete)


# ---- 2. GLM node --------------------------------------------------------------------------------------------------------------
# one P per branch of the layout switch (lpr, ch) = (1,1) (1,2) (1,4) (2,4) (4,4) (8,4) (16,4) (32,3) (32,4) (64,3) (64,4); 300 rows
GLM_P = [1, 3, 8, 9, 24, 40, 100, 130, 200, 300, 512]
GLM_WIDTH = [2, 4, 8, 16, 32, 64, 128, 192, 256, 384, 512]     # 2 lpr ch: the layout each P must select
GLM_FAMILY = ["normal", "bernoulli", "poisson"]


@pytest.mark.parametrize("k", range(len(GLM_P)))
def test_glm_in_every_layout_against_the_restatement(k, monkeypatch):
    P, family = GLM_P[k], GLM_FAMILY[k % 3]
    for v in tl.SCHED_VARS:
        monkeypatch.delenv(v, raising=False)
    spec = tl.glm_model(family, P, 300, k % 2 == 0, "var", False)
    S = (1, 8, 9, 21)[k % 4]
    q = tl._draws(spec, S, seed=P)
    f = tl._vg(spec)
    try:
        assert f.model_scalar("glm_layout_width") == GLM_WIDTH[k]
        got = f.posterior_predictive("y", q, seed=SEED)
    finally:
        f.close()
    want, margin, discrete = ref_glm(spec, q, SEED)
    _hold(f"glm {family} P={P} S={S}", got, want, margin, discrete)
    monkeypatch.setenv("NUTS_LL_B", "1")
    f = tl._vg(spec)
    try:
        assert np.array_equal(f.posterior_predictive("y", q, seed=SEED), got), "NUTS_LL_B=1 against 8"
    finally:
        f.close()


# ---- 3. hierarchical-logit rows -----------------------------------------------------------------------------------------------
ROWS_SIZES = [1, 127, 0, 128, 129, 300, 257, 60, 90, 33, 2] * 6      # unequal groups, empty ones; 66 groups: the group-block pass takes them
ROWS_LAYOUTS = (("general", {"NUTS_ROWS_GA": "0"}, (0.0, False)), ("ga", {"NUTS_ROWS_GA": "2"}, (1.0, False)), ("gb", {"NUTS_ROWS_GB": "1"}, (1.0, True)))


def test_rows_under_every_layout_are_the_same_and_in_the_callers_order(monkeypatch):
    outs = {}
    for label, env, (aligned, block) in ROWS_LAYOUTS:
        for v in tl.SCHED_VARS:
            monkeypatch.delenv(v, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        spec, X, y, gidx = tl.rows_model(ROWS_SIZES, 8, True)
        q = tl._draws(spec, B + 1, seed=31)
        f = tl._vg(spec)
        try:
            assert f.model_scalar("rows_group_aligned") == aligned and (f.model_scalar("rows_group_block") > 0) == block, label
            outs[label] = (f.posterior_predictive("y", q, seed=SEED), predictive.sample_posterior_predictive(spec, q[None], random_seed=SEED, func=f)["y"][0])
        finally:
            f.close()
    want, margin = ref_rows(spec, q, X, gidx, SEED)
    _hold("rows", outs["general"][0], want, margin, True)
    for label in ("ga", "gb"):
        assert np.array_equal(outs[label][0], outs["general"][0]) and np.array_equal(outs[label][1], outs["general"][1]), label
    # the caller's order: row order[j] of the caller is row j of the node
    assert np.array_equal(outs["general"][1][:, np.asarray(spec.rows_order)], outs["general"][0])


# ---- 4. mixture node ----------------------------------------------------------------------------------------------------------
def mix_model9(weights, seed=33):
    rng = np.random.default_rng(seed)
    K, N = 9, 700
    y = np.linspace(-4.0, 4.0, K)[rng.integers(0, K, size=N)] + 0.5 * rng.normal(size=N)
    m = ModelBuilder()
    if weights == "dirichlet":
        w = m.Dirichlet("w", np.linspace(1.0, 2.0, K))
    elif weights == "softmax":
        w = ("softmax", m.Normal("logits", 0.0, 1.0, shape=K))
    else:
        w = rng.dirichlet(np.ones(K) * 3.0)
    mu = m.Normal("mu", 0.0, 10.0, shape=K)
    sigma = m.HalfNormal("sigma", 2.0, shape=K) if weights != "const" else 0.9
    m.NormalMixture("y", w, mu, sigma, y)
    return m.build()


@pytest.mark.parametrize("K", [3, 9])
@pytest.mark.parametrize("weights", ["const", "softmax", "dirichlet"])
def test_marginal_mixture_against_the_restatement(weights, K):
    spec = mix_model9(weights) if K == 9 else tl.mix_model(weights)
    assert spec.mixture_rows.K == K
    q = tl._draws(spec, B + 1, seed=34)
    got = predictive.sample_posterior_predictive(spec, q[None], random_seed=SEED, device=0)["y"][0]
    want, margin = ref_mix(spec, q, SEED)
    keep = margin > 1e-9
    print(weights, K, "left out", int((~keep).sum()), "max abs err", float(np.abs(got[keep] - want[keep]).max()))
    assert (~keep).sum() * 1000 <= keep.size
    np.testing.assert_allclose(got[keep], want[keep], **TOL)


# ---- 5. addressing: batches, splits, seeds, nodes -----------------------------------------------------------------------------
def _nodes_of_every_kernel():
    yield "factor", factor_model(257), "y_gamma"
    yield "factor_derived", derived_model(), "y_side"
    yield "glm", tl.glm_model("poisson", 130, 65, True, None, False), "y"
    yield "rows", tl.rows_model(tl.RAGGED, 8, True)[0], "y"
    yield "mixture", tl.mix_model("dirichlet"), "y"


def test_a_replicate_does_not_depend_on_batch_or_split():
    """S = 21 draws at once, against 5 + 8 + the rest, against one at a time with draw0 -- bit for bit."""
    S = 21
    for label, spec, name in _nodes_of_every_kernel():
        f = tl._vg(spec)
        try:
            q = tl._draws(spec, S, seed=41)
            together = f.posterior_predictive(name, q, seed=SEED)
            parts = np.concatenate([f.posterior_predictive(name, q[a:b], seed=SEED, draw0=a) for a, b in ((0, 5), (5, 13), (13, S))])
            assert np.array_equal(parts, together), label
            for s in range(S):
                assert np.array_equal(f.posterior_predictive(name, q[s : s + 1], seed=SEED, draw0=s)[0], together[s]), (label, s)
            assert not np.array_equal(f.posterior_predictive(name, q[:1], seed=SEED, draw0=1)[0], together[0]), label
            assert not np.array_equal(f.posterior_predictive(name, q, seed=SEED + 1), together), label
        finally:
            f.close()


def test_two_observed_nodes_of_one_model_draw_from_different_streams():
    rng = np.random.default_rng(42)
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    m.Normal("y1", a, 1.0, observed=rng.normal(size=64))
    m.Normal("y2", a, 1.0, observed=rng.normal(size=64))
    spec = m.build()
    got = predictive.sample_posterior_predictive(spec, tl._draws(spec, 3, seed=43)[None], random_seed=SEED, device=0)
    assert not np.any(got["y1"] == got["y2"])


def test_invalid_parameters_give_nan_for_the_element_and_a_failed_check_for_the_row():
    rng = np.random.default_rng(44)
    shift = np.linspace(-1.0, 1.0, 7)
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0)
    s = m.HalfNormal("s", 1.0, transform=None)       # untransformed: a draw may be negative
    m.Normal("y_elem", mu, s + m.as_expr(shift), observed=rng.normal(size=7))
    m.Normal("y_check", mu, m.math.check(m.math.abs(s), m.math.gt(s, 0.0)), observed=rng.normal(size=7))
    spec = m.build()
    q = np.array([[0.1, 1.8], [0.2, 0.3], [-0.4, -0.3]])
    got = predictive.sample_posterior_predictive(spec, q[None], random_seed=SEED, device=0)
    nodes = {nd[0]: nd for nd in ms.observed_nodes(spec)}
    want, margin = ref_factor(spec, nodes["y_elem"][2], q, SEED)
    assert np.array_equal(np.isnan(want), q[:, 1:2] + shift[None, :] <= 0) and np.isnan(want).sum() in range(1, 21)
    _hold("y_elem", got["y_elem"][0], want, margin, False)
    want, margin = ref_factor(spec, nodes["y_check"][2], q, SEED)
    assert np.all(np.isnan(want[2])) and not np.any(np.isnan(want[:2]))
    _hold("y_check", got["y_check"][0], want, margin, False)


# ---- 6. streaming checks ------------------------------------------------------------------------------------------------------
def _summaries(yrep, y):
    """NumPy on the matrix, the sums in extended precision so that the reference's own rounding stays out of the 1e-12"""
    w = yrep.astype(np.longdouble)
    T = np.stack([w.sum(1).astype("float64"), (w ** 2).sum(1).astype("float64"), yrep.min(1), yrep.max(1)], axis=1)
    return w.mean(0).astype("float64"), w.var(0).astype("float64"), (yrep < y).sum(0).astype("float64"), (yrep == y).sum(0).astype("float64"), T


def _accumulator_nodes():
    spec = tl.glm_model("poisson", 9, 300, True, None, False)
    yield "glm poisson", spec, "y", spec.glm_rows.y
    spec = tl.glm_model("normal", 40, 300, True, "var", False)
    yield "glm normal", spec, "y", spec.glm_rows.y
    spec, X, y, gidx = tl.rows_model(ROWS_SIZES, 3, False)
    yield "rows", spec, "y", y[np.asarray(spec.rows_order)].astype("float64")
    spec = factor_model(257)
    yield "factor", spec, "y_poisson", spec.data[spec.factors[next(nd[2] for nd in ms.observed_nodes(spec) if nd[0] == "y_poisson")].args[0].a.ref]
    spec = tl.mix_model("softmax")
    yield "mixture", spec, "y", spec.mixture_rows.y


def test_accumulators_match_numpy_on_the_matrix_and_do_not_depend_on_the_split():
    S = 37
    for label, spec, name, y in _accumulator_nodes():
        q = tl._draws(spec, S, seed=51)
        f = tl._vg(spec)
        try:
            yrep = f.posterior_predictive(name, q, seed=SEED)
            a1, a2 = f.ppc_accumulator(name, seed=SEED), f.ppc_accumulator(name, seed=SEED)
            s0 = 0
            for k in (1, 7, 16, 13):
                a1.update(q[s0 : s0 + k])
                s0 += k
            a2.update(q)
            r1, r2, t1, t2 = a1.read(), a2.read(), a1.stats(), a2.stats()
            a1.close()
            a2.close()
        finally:
            f.close()
        assert r1[4] == r2[4] == S and t1[0].shape == (S, 4)
        for u, v in zip(r1[:4] + t1, r2[:4] + t2):
            assert np.array_equal(u, v), label + ": the state depends on how the draws were split"
        mean_i, var_i, n_lt, n_eq, T = _summaries(yrep, y)
        assert np.array_equal(r1[2], n_lt) and np.array_equal(r1[3], n_eq), label
        assert np.array_equal(t1[0][:, 2:], T[:, 2:]), label
        yw = y.astype(np.longdouble)
        T_obs = np.array([float(yw.sum()), float((yw ** 2).sum()), y.min(), y.max()])

        def rel(got, want):
            with np.errstate(invalid="ignore", divide="ignore"):
                return float(np.nanmax(np.where(want == got, 0.0, np.abs(got - want) / np.abs(want))))

        print(label, "max relative difference: mean_i", rel(r1[0], mean_i), "var_i", rel(r1[1], var_i), "sum", rel(t1[0][:, 0], T[:, 0]),
              "sum of squares", rel(t1[0][:, 1], T[:, 1]), "T_obs", rel(t1[1][:2], T_obs[:2]),
              "| largest condition number of a draw's sum", float((np.abs(yrep).sum(1) / np.abs(yrep.sum(1))).max()))
        np.testing.assert_allclose(r1[0], mean_i, rtol=1e-12, atol=0, err_msg=label)
        np.testing.assert_allclose(r1[1], var_i, rtol=1e-12, atol=0, err_msg=label)
        np.testing.assert_allclose(t1[0][:, 0], T[:, 0], rtol=1e-12, atol=0, err_msg=label)
        np.testing.assert_allclose(t1[0][:, 1], T[:, 1], rtol=1e-12, atol=0, err_msg=label)
        assert np.array_equal(t1[1][2:], T_obs[2:]), label
        np.testing.assert_allclose(t1[1][:2], T_obs[:2], rtol=1e-12, atol=0, err_msg=label)


def test_ppc_pools_chains_and_is_the_summary_of_the_replicates():
    spec, X, y, gidx = tl.rows_model(tl.RAGGED, 3, False)
    q = tl._draws(spec, 2 * 10, seed=52).reshape(2, 10, spec.n)
    out = predictive.ppc(spec, q, random_seed=SEED, pointwise=True, device=0)
    yrep = predictive.sample_posterior_predictive(spec, q, random_seed=SEED, device=0)["y"].reshape(20, -1)     # the caller's order
    yf = y.astype("float64")
    assert out["n_samples"] == 20 and out["n_data_points"] == y.size
    np.testing.assert_allclose(out["mean_i"], yrep.mean(0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(out["var_i"], yrep.var(0), rtol=1e-12, atol=0)
    assert np.array_equal(out["p_i"], ((yrep < yf).sum(0) + 0.5 * (yrep == yf).sum(0)) / 20.0)
    np.testing.assert_allclose(out["T_mean"], yrep.mean(1), rtol=1e-12)
    np.testing.assert_allclose(out["T_sd"], yrep.std(1), rtol=1e-9)
    assert np.array_equal(out["T_min"], yrep.min(1)) and np.array_equal(out["T_max"], yrep.max(1))
    assert out["p_mean"] == float(np.mean(out["T_mean"] >= out["T_obs"]["mean"])) and 0.0 <= out["p_mean"] <= 1.0
    np.testing.assert_allclose(out["T_obs"]["mean"], yf.mean(), rtol=1e-12)


def test_nan_replicates_are_not_hidden_by_the_summaries():
    """An element with invalid parameters at one draw: that draw's four statistics and that observation's mean, variance and p are NaN,
    so are the four p-values; the other draws and observations are what NumPy gives."""
    rng = np.random.default_rng(53)
    shift = np.linspace(-1.0, 1.0, 7)
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0)
    s = m.HalfNormal("s", 1.0, transform=None)
    y = rng.normal(size=7)
    m.Normal("y", mu, s + m.as_expr(shift), observed=y)
    spec = m.build()
    q = np.array([[0.1, 1.8], [0.2, 0.3], [-0.4, 1.2]])      # draw 1: sigma <= 0 for the first elements
    f = tl._vg(spec)
    try:
        yrep = f.posterior_predictive("y", q, seed=SEED)
        acc = f.ppc_accumulator("y", seed=SEED)
        acc.update(q)
        mean_i, var_i, n_lt, n_eq, n = acc.read()
        T, T_obs = acc.stats()
        acc.close()
    finally:
        f.close()
    bad = np.isnan(yrep)
    assert bad[1].any() and not bad[[0, 2]].any() and not bad[:, -1].any()
    assert np.all(np.isnan(T[1])) and not np.any(np.isnan(T[[0, 2]])) and not np.any(np.isnan(T_obs))
    assert np.array_equal(T[[0, 2], 2:], np.stack([yrep[[0, 2]].min(1), yrep[[0, 2]].max(1)], axis=1))
    assert np.array_equal(np.isnan(mean_i), bad.any(0)) and np.array_equal(np.isnan(var_i), bad.any(0))
    out = predictive.ppc_from_accumulators(mean_i, var_i, n_lt, n_eq, T, T_obs, n, pointwise=True)
    assert np.array_equal(np.isnan(out["p_i"]), bad.any(0)) and all(np.isnan(out["p_" + k]) for k in predictive.STATS)
    ok = ~bad.any(0)
    assert np.array_equal(out["p_i"][ok], ((yrep < y).sum(0) + 0.5 * (yrep == y).sum(0))[ok] / 3.0)


# ---- 7. the public interface --------------------------------------------------------------------------------------------------
def test_sample_returns_the_posterior_predictive_group_on_request():
    from pymc_amd.sampling import sample

    spec = models.eight_schools()
    res = sample(draws=20, tune=20, chains=2, model=spec, random_seed=19, device=0, posterior_predictive=True)
    try:
        pp = res["posterior_predictive"]
        assert list(pp) == ["obs"] and pp["obs"].shape == (2, 20, 8) and np.all(np.isfinite(pp["obs"]))
        again = predictive.sample_posterior_predictive(spec, res, random_seed=predictive.seed_from(19), device=0)
        assert np.array_equal(again["obs"], pp["obs"])
        fi = ms.observed_nodes(spec)[0][2]
        want, margin = ref_factor(spec, fi, res["draws"].reshape(40, -1), predictive.seed_from(19))
        _hold("obs", pp["obs"].reshape(40, 8), want, margin, False)
    finally:
        res["step"].close()
    res = sample(draws=5, tune=5, chains=1, model=spec, random_seed=19, device=0)
    assert "posterior_predictive" not in res
    res["step"].close()


def test_the_engine_refuses_by_name_what_is_out_of_scope():
    spec = tl.factor_model(7)
    f = tl._vg(spec)
    try:
        nodes = {nd[0]: nd for nd in ms.observed_nodes(spec)}
        with pytest.raises(Exception, match="Binomial is out of scope"):
            f.posterior_predictive("y_binomial", np.zeros((1, spec.n)))
        with pytest.raises(ValueError, match="Binomial is out of scope"):
            f.ppc_accumulator("y_binomial")
        with pytest.raises(Exception, match="below 2\\^32"):
            f.posterior_predictive("y_normal", np.zeros((2, spec.n)), draw0=2 ** 32 - 1)
        assert f.posterior_predictive("y_normal", np.zeros((1, spec.n)), draw0=2 ** 32 - 1).shape == (1, 7)
        assert nodes["y_binomial"][1] == ms.LL_FACTOR
    finally:
        f.close()
    with pytest.raises(ValueError, match="Binomial"):
        predictive.sample_posterior_predictive(spec, np.zeros((1, 1, spec.n)), device=0)


def test_the_engine_refuses_a_factor_whose_value_is_an_expression_of_variables():
    """y_i - t ~ HalfNormal(1) (tests/test_gpu_loglik.py builds it for the -inf case): there is no observed vector to replicate"""
    m = ModelBuilder()
    t = m.Normal("t", 0.0, 1.0)
    m.spec.data.append(np.array([0.1, 3.0, 4.0]))
    value = ms.Term(ms.Operand(ms.OP_DATA, 0.0, len(m.spec.data) - 1), ms.Operand(ms.OP_CONST, -1.0), t.term.a)
    m.spec.factors.append(ms.Factor(ms.D_HALFNORMAL, 3, (value, ms.Term(ms.Operand(ms.OP_CONST, 1.0))), 0.0, "y", (), observed=True))
    spec = m.build()
    assert "expression of variables" in predictive.refusal(spec)
    f = tl._vg(spec)
    try:
        with pytest.raises(Exception, match="expression of variables"):
            f.posterior_predictive("y", np.zeros((1, spec.n)))
        with pytest.raises(ValueError, match="expression of variables"):
            f.ppc_accumulator("y")
        assert f.log_likelihood("y", np.zeros((1, spec.n))).shape == (1, 3)      # (the log-likelihood of such a factor stays available)
    finally:
        f.close()


def test_draws_are_numbered_by_the_models_chain_numbers():
    """A process that holds only chain 1 of two draws what the process holding both draws for it."""
    spec = tl.glm_model("poisson", 9, 300, True, None, False)
    q = tl._draws(spec, 2 * 5, seed=61).reshape(2, 5, spec.n)
    both = predictive.sample_posterior_predictive(spec, q, random_seed=SEED, device=0)["y"]
    alone = predictive.sample_posterior_predictive(spec, {"draws": q[1:2], "chains": [1]}, random_seed=SEED, device=0)["y"]
    assert np.array_equal(alone[0], both[1]) and not np.array_equal(both[0], both[1])
    assert np.array_equal(predictive.sample_posterior_predictive(spec, q[1:2], random_seed=SEED, chain_ids=[1], device=0)["y"], alone)
    with pytest.raises(ValueError, match="chain_ids"):
        predictive.sample_posterior_predictive(spec, q, chain_ids=[0], device=0)


def test_chain_group_member_is_refused():
    from pymc_amd.chain_group import ChainGroup
    from pymc_amd.sampling import init_nuts

    spec = models.mvnormal(n=256, seed=5)
    step = init_nuts(spec, init="adapt_diag", chains=1, random_seed_list=[1], device=0, tune=10)[1]
    group = ChainGroup([step])
    try:
        with pytest.raises(ValueError, match="chain group"):
            step._logp_dlogp_func.posterior_predictive("x", np.zeros((1, spec.n)), node=(ms.LL_FACTOR, 0))
    finally:
        group.close()
        step.close()
