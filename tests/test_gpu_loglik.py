"""Pointwise log-likelihood on the device (csrc/loglik_kernel.h, pymc_amd/loglik.py) against the oracle, and the streaming WAIC.

Reference: for element-wise factors `oracle.ref_models.backward` + `_forward` + `_dist` (the per-element values the joint log-density
sums); for the three dense nodes the formulas of `_glm_rows` / `_logit_rows` / `_mixture_rows` before their `sum`, restated below.
Bars: pointwise values rtol = atol = 1e-10 (the bar device log-densities are held to against the oracle), the reduced WAIC quantities
1e-9.  Inputs are seeded, unconstrained draws ~ N(0, 0.5^2), covariates scaled so that |eta| <= 5: every reference value is finite
(asserted) and no element is left out of a comparison.
"""

import os
import sys

import numpy as np
import pytest
from scipy.special import gammaln, logsumexp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import ref_models  # noqa: E402
from pymc_amd import loglik, models  # noqa: E402
from pymc_amd import model_spec as ms  # noqa: E402
from pymc_amd.model_spec import ModelBuilder  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-10, atol=1e-10)
B = 8      # draws per batch (asserted against the engine's own figure in test_batch_size_is_what_the_tests_assume)
SCHED_VARS = ("NUTS_ROWS_GA", "NUTS_ROWS_GB", "NUTS_GA_AUX", "NUTS_ROWS_GA_W", "NUTS_FOLD_CTL", "NUTS_LEAN_STRICT", "NUTS_LL_B")


def _vg(spec):
    from pymc_amd.value_grad import DeviceValueGradFunction

    return DeviceValueGradFunction(spec, device=0)


def _draws(spec, S, seed):
    return np.random.default_rng(seed).normal(size=(S, spec.n)) * 0.5


def _constrained(spec, q):
    x = np.empty(spec.n)
    for v in spec.vars:
        sl = slice(v.offset, v.offset + v.size)
        x[sl] = ref_models.backward(v.transform, q[sl], v.lower, v.upper)[0]
    return x


def ref_factor(spec, fi, q):
    """[S, size]: the oracle's per-element log-density of factor fi at every draw."""
    f = spec.factors[fi]
    out = np.empty((len(q), f.size))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s, qs in enumerate(q):
            x = _constrained(spec, qs)
            derived = {i: np.broadcast_to(ref_models._forward(spec, g, x)[0][0], (g.size,)) for i, g in enumerate(spec.factors) if g.dist == ms.D_DERIVED}
            args, _, _, _, dead = ref_models._forward(spec, f, x, derived)
            lp, _ = ref_models._dist(f.dist, f.konst, args)
            out[s] = -np.inf if dead else np.broadcast_to(lp, (f.size,))
    return out


def _log_sigmoid_rows(eta, y):
    return np.where(y != 0, -np.logaddexp(0.0, -eta), -np.logaddexp(0.0, eta))


def ref_glm(spec, q):
    node = spec.glm_rows
    out = np.empty((len(q), node.y.size))
    for s, qs in enumerate(q):
        x = _constrained(spec, qs)
        if node.beta is not None:
            v = spec.vars[node.beta]
            beta = x[v.offset : v.offset + v.size]
        else:
            beta = np.broadcast_to(ref_models._forward(spec, spec.factors[node.beta_derived], x)[0][0], (node.X.shape[1],))
        eta = node.X @ beta + (x[spec.vars[node.intercept].offset] if node.intercept is not None else 0.0)
        if node.family == ms.GLM_NORMAL:
            sigma = x[spec.vars[node.sigma].offset] if node.sigma is not None else node.sigma_const
            z = (node.y - eta) / sigma
            out[s] = -0.5 * z * z - np.log(np.sqrt(2.0 * np.pi)) - np.log(sigma)
        elif node.family == ms.GLM_BERNOULLI:
            out[s] = _log_sigmoid_rows(eta, node.y)
        else:
            out[s] = node.y * eta - gammaln(node.y + 1.0) - np.exp(eta)
        assert np.abs(eta).max() <= 5.0
    return out


def ref_rows(spec, q, X, y, gidx):
    """In the CALLER's row order (X, y, gidx as passed to the builder)."""
    node = spec.logit_rows
    vm, vs, vz = (spec.vars[i] for i in (node.mu, node.sigma, node.z))
    D = vm.size
    out = np.empty((len(q), len(y)))
    for s, qs in enumerate(q):
        x = _constrained(spec, qs)
        beta = x[vm.offset : vm.offset + D] + x[vs.offset : vs.offset + D] * x[vz.offset : vz.offset + vz.size].reshape(-1, D)
        eta = np.einsum("nd,nd->n", X, beta[gidx])
        assert np.abs(eta).max() <= 5.0
        out[s] = _log_sigmoid_rows(eta, y)
    return out


def ref_mix(spec, q):
    node = spec.mixture_rows
    K = node.K
    out = np.empty((len(q), node.y.size))
    for s, qs in enumerate(q):
        x = _constrained(spec, qs)
        mu = x[spec.vars[node.mu].offset :][:K]
        sigma = x[spec.vars[node.sigma].offset :][:K] if node.sigma is not None else np.asarray(node.sigma_const)
        if node.w_alpha is not None:
            yv = x[spec.vars[node.w_logits].offset :][: K - 1]
            eta = np.concatenate([yv, [-yv.sum()]])
            logw = eta - logsumexp(eta)
        elif node.w_logits is not None:
            eta = x[spec.vars[node.w_logits].offset :][:K]
            logw = eta - logsumexp(eta)
        else:
            logw = np.log(node.w_const)
        comp = -0.5 * ((node.y[:, None] - mu) / sigma) ** 2 - np.log(np.sqrt(2.0 * np.pi)) - np.log(sigma)
        out[s] = logsumexp(logw + comp, axis=1)
    return out


def test_batch_size_is_what_the_tests_assume():
    f = _vg(models.eight_schools())
    assert f.model_scalar("loglik_batch") == B
    assert f.model_scalar("loglik_stage_bytes") == 0
    f.close()


# ---- 1. element-wise factors --------------------------------------------------------------------------------------------------
def factor_model(N, seed=1):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=N)
    idx = rng.integers(0, 5, size=N)
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    b = m.Normal("b", 0.0, 1.0)
    s = m.HalfNormal("s", 1.0)
    loc = m.Normal("loc", 0.0, 1.0, shape=N)
    g = m.Normal("g", 0.0, 1.0, shape=5)
    m.Normal("y_normal", loc, s, observed=rng.normal(size=N))
    m.Poisson("y_poisson", m.math.exp(a + b * m.as_expr(x)), observed=rng.poisson(1.5, size=N).astype("float64"))
    m.Binomial("y_binomial", 10.0, m.math.sigmoid(a + b * m.as_expr(x)), observed=rng.integers(0, 11, size=N).astype("float64"))
    m.StudentT("y_studentt", 4.0, a + b * m.as_expr(x), s, observed=rng.normal(size=N))
    m.Normal("y_gather", g[idx], 1.0, observed=rng.normal(size=N))
    return m.build()


@pytest.mark.parametrize("N", [1, 255, 257, 1000])
def test_factors_against_the_oracle(N):
    spec = factor_model(N)
    nodes = ms.observed_nodes(spec)
    assert [nd[0] for nd in nodes] == ["y_normal", "y_poisson", "y_binomial", "y_studentt", "y_gather"]
    q = _draws(spec, 5, seed=N)
    got = loglik.compute_log_likelihood(spec, q[None], device=0)
    for name, kind, index, size in nodes:
        ref = ref_factor(spec, index, q)
        assert size == N and np.all(np.isfinite(ref))
        print(name, N, "max abs err", np.abs(got[name][0] - ref).max())
        np.testing.assert_allclose(got[name][0], ref, err_msg=name, **TOL)


def test_observed_variable_lowered_op_by_op():
    """An observed RV without a distribution code of its own -- StudentT with a variable nu: a D_POTENTIAL factor whose term is the
    per-element log-density."""
    import more_models as tm
    import stubgraph as sg
    from pymc_amd.lowering import lower_to_spec

    model = sg.FrozenModel(sg.load_models(tm.FIXTURE)["stochastic_volatility"])
    model.logp_observed = [nm == "returns" for nm in model.logp_names]
    spec = lower_to_spec(model)
    nodes = ms.observed_nodes(spec)
    assert [nd[0] for nd in nodes] == ["returns"] and nodes[0][3] == tm.T_SV
    assert spec.factors[nodes[0][2]].dist == ms.D_POTENTIAL
    q = _draws(spec, 5, seed=2)
    got = loglik.compute_log_likelihood(spec, q[None], device=0)["returns"][0]
    ref = ref_factor(spec, nodes[0][2], q)
    assert np.all(np.isfinite(ref))
    np.testing.assert_allclose(got, ref, **TOL)


def _softmax_lin_spec():
    spec = models.softmax_regression(N=1030, P=4, K=3, seed=3, lin=True)
    assert spec.lins, "the model must go through the linear-predictor node"
    fi = next(i for i, f in enumerate(spec.factors) if f.name == "y")
    spec.factors[fi].observed = True      # (a Potential of the builder: the test says it is the likelihood)
    return spec, fi


def test_factor_that_reads_linear_predictors():
    spec, fi = _softmax_lin_spec()
    q = _draws(spec, 3, seed=4)
    got = loglik.compute_log_likelihood(spec, q[None], device=0)["y"][0]
    ref = ref_factor(spec, fi, q)
    assert ref.shape == (3, 1030) and np.all(np.isfinite(ref))
    np.testing.assert_allclose(got, ref, **TOL)


def test_failed_parameter_check_kills_the_factor_at_that_draw_only():
    rng = np.random.default_rng(5)
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0)
    s = m.HalfNormal("s", 1.0, transform=None)       # untransformed: a draw may be negative
    m.Normal("y", mu, s, observed=rng.normal(size=7))
    spec = m.build()
    q = np.array([[0.1, 0.8], [0.2, -0.3], [-0.4, 1.2]])
    got = loglik.compute_log_likelihood(spec, q[None], device=0)["y"][0]
    ref = ref_factor(spec, ms.observed_nodes(spec)[0][2], q)
    assert np.all(np.isneginf(ref[1])) and np.all(np.isfinite(ref[[0, 2]]))
    assert np.all(np.isneginf(got[1]))
    np.testing.assert_allclose(got[[0, 2]], ref[[0, 2]], **TOL)


# ---- 2. GLM node --------------------------------------------------------------------------------------------------------------
def glm_model(family, P, N, intercept, sigma, derived, seed=7):
    rng = np.random.default_rng(seed + P + N)
    X = rng.normal(size=(N, P)) / np.sqrt(P)
    if family == "normal":
        y = rng.normal(size=N)
    elif family == "bernoulli":
        y = (rng.random(N) < 0.5).astype("float64")
    else:
        y = rng.poisson(2.0, size=N).astype("float64")
    m = ModelBuilder()
    alpha = m.Normal("alpha", 0.0, 5.0) if intercept else None
    if derived:
        mu0 = m.Normal("mu0", 0.0, 1.0)
        tau = m.HalfNormal("tau", 1.0)
        z = m.Normal("z", 0.0, 1.0, shape=P)
        beta = mu0 + tau * z
    else:
        beta = m.Normal("beta", 0.0, 1.0, shape=P)
    sg = 1.0
    if family == "normal":
        sg = m.HalfNormal("sigma", 1.0) if sigma == "var" else 0.8
    m.GLM("y", X, beta, y, family=family, intercept=alpha, sigma=sg)
    return m.build()


# every (lpr, ch) layout, odd P, rows that read on into the next row; wave ranges with none / partial / full iterations; batches of
# 1, B - 1, B + 1, 2 B + 3; each family; intercept present / absent; sigma variable / constant; one derived beta
GLM_CASES = [
    ("normal", 1, 1, 1, True, "var", False),
    ("normal", 3, 63, B - 1, False, "const", False),
    ("bernoulli", 8, 65, B + 1, True, None, False),
    ("poisson", 9, 1000, 2 * B + 3, True, None, False),
    ("bernoulli", 65, 63, B - 1, False, None, False),
    ("normal", 130, 65, B + 1, True, "var", False),
    ("poisson", 512, 65, 1, False, None, False),
    ("bernoulli", 512, 1000, B + 1, True, None, False),
    ("normal", 9, 1000, 2 * B + 3, False, "const", True),
    ("poisson", 3, 1, B - 1, True, None, False),
    ("bernoulli", 1, 1000, 2 * B + 3, False, None, False),
    ("normal", 65, 1000, B - 1, False, "var", False),
    ("poisson", 130, 63, B + 1, True, None, False),
]


@pytest.mark.parametrize("family,P,N,S,intercept,sigma,derived", GLM_CASES)
def test_glm_against_numpy(family, P, N, S, intercept, sigma, derived):
    spec = glm_model(family, P, N, intercept, sigma, derived)
    assert (spec.glm_rows.beta is None) == derived
    q = _draws(spec, S, seed=P * 1000 + N)
    got = loglik.compute_log_likelihood(spec, q[None], device=0)["y"][0]
    ref = ref_glm(spec, q)
    assert got.shape == (S, N) and np.all(np.isfinite(ref))
    print(family, P, N, S, "max abs err", np.abs(got - ref).max())
    np.testing.assert_allclose(got, ref, **TOL)


# ---- 3. hierarchical-logit rows -----------------------------------------------------------------------------------------------
def rows_model(sizes, D, ones, seed=9):
    """Ragged groups, rows passed UNSORTED."""
    rng = np.random.default_rng(seed)
    G = len(sizes)
    gidx = np.repeat(np.arange(G, dtype="int32"), sizes)
    N = gidx.size
    X = rng.normal(size=(N, D)) * (0.5 / np.sqrt(D))
    if ones:
        X[:, 0] = 1.0
    y = (rng.random(N) < 0.5).astype("int8")
    perm = rng.permutation(N)
    X, y, gidx = X[perm], y[perm], gidx[perm]
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0, shape=D)
    sigma = m.HalfNormal("sigma", 1.0, shape=D)
    z = m.Normal("z", 0.0, 1.0, shape=(G, D))
    m.HierLogitRows("y", X, y, gidx, mu, sigma, z)
    return m.build(), X, y, gidx


RAGGED = [1, 127, 128, 129, 300, 257]
ROWS_LAYOUTS = {
    # group-aligned forced on a small model; group-block by default from 64 groups on; the span-tiled general path below that
    "ga": dict(sizes=RAGGED * 2, env={"NUTS_ROWS_GA": "2"}, expect={"rows_group_aligned": 1.0, "rows_group_block": 0.0}),
    "gb": dict(sizes=(RAGGED + [60, 90, 33, 2]) * 8, env={}, expect={"rows_group_aligned": 1.0, "rows_group_block": True}),
    "general": dict(sizes=RAGGED * 3, env={}, expect={"rows_group_aligned": 0.0, "rows_group_block": 0.0}),
}


@pytest.mark.parametrize("D,ones", [(8, True), (3, False)])
@pytest.mark.parametrize("layout", list(ROWS_LAYOUTS))
def test_rows_in_every_layout_in_the_callers_order(layout, D, ones, monkeypatch):
    for k in SCHED_VARS:
        monkeypatch.delenv(k, raising=False)
    lay = ROWS_LAYOUTS[layout]
    for k, v in lay["env"].items():
        monkeypatch.setenv(k, v)
    spec, X, y, gidx = rows_model(lay["sizes"], D, ones)
    assert spec.rows_order is not None
    f = _vg(spec)
    try:
        for k, want in lay["expect"].items():
            got = f.model_scalar(k)
            assert ((got > 0) == (want > 0)) if isinstance(want, bool) else got == want, (k, got, want)
        q = _draws(spec, B + 1, seed=D)
        got = loglik.compute_log_likelihood(spec, q[None], func=f)["y"][0]
    finally:
        f.close()
    ref = ref_rows(spec, q, X, y, gidx)
    assert np.all(np.isfinite(ref))
    print(layout, D, "max abs err", np.abs(got - ref).max())
    np.testing.assert_allclose(got, ref, **TOL)


# ---- 4. mixture node, marginal form -------------------------------------------------------------------------------------------
def mix_model(weights, seed=11):
    rng = np.random.default_rng(seed)
    K, N = 3, 1000
    y = np.linspace(-2.0, 2.0, K)[rng.integers(0, K, size=N)] + 0.7 * rng.normal(size=N)
    m = ModelBuilder()
    if weights == "dirichlet":
        w = m.Dirichlet("w", np.array([1.5, 2.0, 1.0]))
    elif weights == "softmax":
        w = ("softmax", m.Normal("logits", 0.0, 1.0, shape=K))
    else:
        w = np.array([0.2, 0.5, 0.3])
    mu = m.Normal("mu", 0.0, 10.0, shape=K)
    sigma = m.HalfNormal("sigma", 2.0, shape=K) if weights != "const" else 0.9
    m.NormalMixture("y", w, mu, sigma, y)
    return m.build()


@pytest.mark.parametrize("weights", ["const", "softmax", "dirichlet"])
def test_marginal_mixture_against_numpy(weights):
    spec = mix_model(weights)
    q = _draws(spec, B + 1, seed=12)
    got = loglik.compute_log_likelihood(spec, q[None], device=0)["y"][0]
    ref = ref_mix(spec, q)
    assert got.shape == (B + 1, 1000) and np.all(np.isfinite(ref))
    np.testing.assert_allclose(got, ref, **TOL)


# ---- 5. batch independence ----------------------------------------------------------------------------------------------------
def _four_kernels():
    yield "factor", factor_model(257), "y_studentt"
    yield "factor_lin", _softmax_lin_spec()[0], "y"
    yield "glm", glm_model("poisson", 130, 65, True, None, False), "y"
    yield "rows", rows_model(RAGGED, 8, True)[0], "y"
    yield "mixture", mix_model("dirichlet"), "y"


def test_a_draw_does_not_depend_on_its_batch():
    """loglik(q)[s] is BITWISE loglik(q[s : s + 1])[0] for every s of a ragged batch (B + 3 draws: a full batch and a partial one)."""
    for label, spec, name in _four_kernels():
        f = _vg(spec)
        try:
            q = _draws(spec, B + 3, seed=13)
            together = f.log_likelihood(name, q)
            for s in range(len(q)):
                alone = f.log_likelihood(name, q[s : s + 1])[0]
                assert np.array_equal(together[s], alone), (label, s)
        finally:
            f.close()


# ---- 6. streaming WAIC --------------------------------------------------------------------------------------------------------
def _two_pass(ll):
    S = ll.shape[0]
    lppd_i = logsumexp(ll, axis=0) - np.log(S)
    p_i = np.var(ll, axis=0)
    elpd_i = lppd_i - p_i
    return lppd_i, p_i, float(elpd_i.sum()), float(np.sqrt(elpd_i.size * np.var(elpd_i)))


def test_streaming_waic_matches_two_pass_numpy_and_never_holds_the_matrix():
    spec = glm_model("bernoulli", 9, 257, True, None, False)
    S, N = 37, 257
    q = _draws(spec, S, seed=14)
    f = _vg(spec)
    try:
        a1 = f.waic_accumulator("y")
        a2 = f.waic_accumulator("y")
        s0 = 0
        for k in (1, 7, 16, 13):
            a1.update(q[s0 : s0 + k])
            s0 += k
        a2.update(q)
        raw1, n1 = a1.raw()
        raw2, n2 = a2.raw()
        lppd_i, p_i, n3 = a1.read()
        a1.close()
        a2.close()
        assert n1 == n2 == n3 == S
        assert np.array_equal(raw1, raw2), "the accumulators depend on how the draws were split"
        # no S x N buffer: the one block of values the model holds is [batch][N]
        assert f.model_scalar("loglik_stage_bytes") == B * N * 8 < S * N * 8
        out = loglik.waic(spec, q[None], pointwise=True, func=f)
    finally:
        f.close()
    ref_l, ref_p, ref_elpd, ref_se = _two_pass(ref_glm(spec, q))
    np.testing.assert_allclose(lppd_i, ref_l, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(p_i, ref_p, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(out["lppd_i"], ref_l, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(out["p_waic_i"], ref_p, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(out["elpd_waic"], ref_elpd, rtol=1e-9)
    np.testing.assert_allclose(out["se"], ref_se, rtol=1e-9)
    assert out["n_samples"] == S and out["n_data_points"] == N
    assert out["warning"] == bool(np.any(ref_p > 0.4))


def test_waic_pools_chains_and_undoes_the_row_order():
    spec, X, y, gidx = rows_model(RAGGED, 3, False)
    q = _draws(spec, 2 * 10, seed=15).reshape(2, 10, spec.n)
    out = loglik.waic(spec, q, pointwise=True, device=0)
    ref_l, ref_p, ref_elpd, ref_se = _two_pass(ref_rows(spec, q.reshape(20, -1), X, y, gidx))
    np.testing.assert_allclose(out["lppd_i"], ref_l, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(out["p_waic_i"], ref_p, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose([out["elpd_waic"], out["se"]], [ref_elpd, ref_se], rtol=1e-9)


def test_minus_infinity_at_some_draws_leaves_lppd_finite():
    """y_i - t ~ HalfNormal(1) with a scalar variable t: observation 0 (y = 0.1) is outside the support at the draws with t > 0.1 and
    inside at the others -- its lppd is the logsumexp of the finite ones, not NaN."""
    m = ModelBuilder()
    t = m.Normal("t", 0.0, 1.0)
    yv = np.array([0.1, 3.0, 4.0])
    m.spec.data.append(yv)
    value = ms.Term(ms.Operand(ms.OP_DATA, 0.0, len(m.spec.data) - 1), ms.Operand(ms.OP_CONST, -1.0), t.term.a)
    m.spec.factors.append(ms.Factor(ms.D_HALFNORMAL, 3, (value, ms.Term(ms.Operand(ms.OP_CONST, 1.0))), 0.0, "y", (), observed=True))
    spec = m.build()
    q = np.array([[-0.5], [0.4], [0.0], [0.9], [-0.2], [0.3], [-1.0], [0.05], [0.6], [-0.1], [0.2]])
    ref = ref_factor(spec, 1, q)
    assert np.any(np.isneginf(ref[:, 0])) and np.any(np.isfinite(ref[:, 0])) and np.all(np.isfinite(ref[:, 1:]))
    f = _vg(spec)
    try:
        got = f.log_likelihood("y", q)
        acc = f.waic_accumulator("y")
        acc.update(q[:4])
        acc.update(q[4:])
        lppd_i, p_i, n = acc.read()
        acc.close()
    finally:
        f.close()
    assert np.array_equal(np.isneginf(got), np.isneginf(ref))
    np.testing.assert_allclose(got, ref, **TOL)
    ref_l = logsumexp(ref, axis=0) - np.log(len(q))
    assert np.all(np.isfinite(lppd_i))
    np.testing.assert_allclose(lppd_i, ref_l, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(p_i[1:], np.var(ref[:, 1:], axis=0), rtol=1e-9, atol=1e-9)


# ---- 7. sum rule --------------------------------------------------------------------------------------------------------------
def _schools(with_obs):
    y = np.array([28, 8, -3, 7, -1, 1, 18, 12], dtype="float64")
    sigma = np.array([15, 10, 16, 11, 9, 11, 10, 18], dtype="float64")
    m = ModelBuilder()
    eta = m.Normal("eta", 0.0, 1.0, shape=8)
    mu = m.Normal("mu", 0.0, 1e6)
    tau = m.HalfCauchy("tau", 25.0)
    if with_obs:
        m.Normal("obs", mu + tau * eta, sigma, observed=y)
    return m.build()


def _glm_pair(with_obs):
    rng = np.random.default_rng(16)
    X = rng.normal(size=(300, 9)) * 0.5
    y = rng.poisson(2.0, size=300).astype("float64")
    m = ModelBuilder()
    alpha = m.Normal("alpha", 0.0, 5.0)
    beta = m.Normal("beta", 0.0, 1.0, shape=9)
    if with_obs:
        m.GLM("y", X, beta, y, family="poisson", intercept=alpha)
    return m.build()


def _rows_pair(with_obs):
    rng = np.random.default_rng(17)
    G, D = 5, 3
    gidx = np.repeat(np.arange(G, dtype="int32"), [1, 127, 128, 129, 40])
    X = rng.normal(size=(gidx.size, D)) * 0.5
    y = (rng.random(gidx.size) < 0.5).astype("int8")
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0, shape=D)
    sigma = m.HalfNormal("sigma", 1.0, shape=D)
    z = m.Normal("z", 0.0, 1.0, shape=(G, D))
    if with_obs:
        m.HierLogitRows("y", X, y, gidx, mu, sigma, z)
    return m.build()


@pytest.mark.parametrize("pair", [_schools, _glm_pair, _rows_pair])
def test_pointwise_values_sum_to_the_likelihoods_share_of_logp(pair):
    """sum(pointwise) + logp(model without its likelihood) = logp(model), through nuts_model_logp_grad: independent of the
    element-wise reference."""
    full, prior = pair(True), pair(False)
    assert full.n == prior.n
    q = _draws(full, 3, seed=18)
    f, g = _vg(full), _vg(prior)
    try:
        name = ms.observed_nodes(full)[0][0]
        ll = f.log_likelihood(name, q)
        for s in range(len(q)):
            lp_full, _ = f._pytensor_function(q[s])
            lp_prior, _ = g._pytensor_function(q[s])
            bound = 1e-10 * (np.abs(ll[s]).sum() + abs(lp_prior))
            assert abs(ll[s].sum() + lp_prior - lp_full) <= bound, (s, ll[s].sum() + lp_prior - lp_full, bound)
    finally:
        f.close()
        g.close()


# ---- 8. sample() --------------------------------------------------------------------------------------------------------------
def test_sample_returns_the_log_likelihood_group_on_request():
    from pymc_amd.sampling import sample

    spec = models.eight_schools()
    res = sample(draws=20, tune=20, chains=2, model=spec, random_seed=19, device=0, log_likelihood=True)
    try:
        ll = res["log_likelihood"]
        assert list(ll) == ["obs"] and ll["obs"].shape == (2, 20, 8)
        again = loglik.compute_log_likelihood(spec, res, device=0)
        assert np.array_equal(again["obs"], ll["obs"])
        fi = ms.observed_nodes(spec)[0][2]
        ref = ref_factor(spec, fi, res["draws"].reshape(40, -1)).reshape(2, 20, 8)
        np.testing.assert_allclose(ll["obs"], ref, **TOL)
    finally:
        res["step"].close()
    res = sample(draws=5, tune=5, chains=1, model=spec, random_seed=19, device=0)
    assert "log_likelihood" not in res
    res["step"].close()


def test_chain_group_member_is_refused():
    """The calls use the model's own stream: refused with a text while the model's chain is a member of a chain group."""
    from pymc_amd.chain_group import ChainGroup
    from pymc_amd.sampling import init_nuts

    spec = models.mvnormal(n=256, seed=5)
    step = init_nuts(spec, init="adapt_diag", chains=1, random_seed_list=[1], device=0, tune=10)[1]
    group = ChainGroup([step])
    try:
        with pytest.raises(ValueError, match="chain group"):
            step._logp_dlogp_func.log_likelihood("x", np.zeros((1, spec.n)), node=(ms.LL_FACTOR, 0))
    finally:
        group.close()
        step.close()
