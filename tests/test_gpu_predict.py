"""Predictions at new data on the device (csrc/predict.h, csrc/predict_kernel.h, pymc_amd/predictive.py `predict`) against the NumPy
restatement (tests/predict_reference.py) fed the reference parameters of tests/test_gpu_loglik.py / tests/test_gpu_predictive.py.

Models and draw scales are those of tests/test_gpu_loglik.py (seeded unconstrained draws ~ N(0, 0.5^2), covariates scaled so that
|eta| <= 5).  Shapes are the smallest at which the kernels change shape: M around LL_BLOCK = 256 (1, 255, 256, 257, 513) and S a lone
draw, a full batch, a ragged batch, two batches and a tail (1, 8, 9, 19).

Bars.  Per-draw moments against the restatement: rtol = atol = 1e-10, the project's bar for device values; NaN and inf patterns equal.
Accumulators against NumPy (sums in extended precision) on the matrix the device returned: rtol 1e-12; the lpd, a difference of O(1)
terms each rounded to a double, also gets atol 1e-15 (a few units in the last place of 1).  var_between + var_within against the
variance of the mixture of the draws computed from its second moment, E[v + m^2] - E[m]^2: rtol 1e-12 plus 1e-12 of that second
moment, the cancellation of the direct formula itself.  Batches and splits: `array_equal`.
"""

import os
import sys

import numpy as np
import pytest
from scipy.special import logsumexp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import predict_reference as ref  # noqa: E402
import test_gpu_loglik as tl  # noqa: E402
import test_gpu_predictive as tp  # noqa: E402
from oracle import ref_models  # noqa: E402
from pymc_amd import loglik, models, predictive  # noqa: E402
from pymc_amd import model_spec as ms  # noqa: E402
from pymc_amd.model_spec import ModelBuilder, data_inputs, with_data  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-10, atol=1e-10)
B = tl.B
SEED = tp.SEED


def _same_pattern(got, want, label):
    assert got.shape == want.shape, label
    assert np.array_equal(np.isnan(got), np.isnan(want)), label + ": NaN pattern"
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), label + ": inf pattern"
    return np.isfinite(want)


def _hold_values(got, want, label):
    fin = _same_pattern(got, want, label)
    print(label, "max abs err", float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0)
    np.testing.assert_allclose(got[fin], want[fin], err_msg=label, **TOL)


# ---- references: the node's parameters at every draw (caller's order), then the restatement ---------------------------------------
def ref_glm(spec, q):
    eta, sigma = tp.glm_parameters(spec, q)
    fam = spec.glm_rows.family
    if fam == ms.GLM_NORMAL:
        return ref.moments(ref.D_NORMAL, eta, sigma[:, None])
    if fam == ms.GLM_BERNOULLI:
        return ref.moments(ref.D_BERNOULLI_LOGIT, eta)
    return ref.moments(ref.D_POISSON, np.exp(eta))


def ref_rows(spec, q, X, gidx):
    node = spec.logit_rows
    vm, vs, vz = (spec.vars[i] for i in (node.mu, node.sigma, node.z))
    D = vm.size
    eta = np.empty((len(q), len(gidx)))
    for s, qs in enumerate(q):
        x = tl._constrained(spec, qs)
        beta = x[vm.offset : vm.offset + D] + x[vs.offset : vs.offset + D] * x[vz.offset : vz.offset + vz.size].reshape(-1, D)
        eta[s] = np.einsum("nd,nd->n", X, beta[gidx])
    assert np.abs(eta).max() <= 5.0
    return ref.moments(ref.D_BERNOULLI_LOGIT, eta)


def ref_factor(spec, fi, q):
    f = spec.factors[fi]
    m, v = np.empty((len(q), f.size)), np.empty((len(q), f.size))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s, qs in enumerate(q):
            x = tl._constrained(spec, qs)
            args, _, _, _, dead = ref_models._forward(spec, f, x, {})
            a = [args[k] if k < len(args) else 0.0 for k in (1, 2, 3)]
            ms_, vs_ = ref.moments(f.dist, a[0], a[1], a[2])
            m[s], v[s] = (np.nan, np.nan) if dead else (np.broadcast_to(ms_, (f.size,)), np.broadcast_to(vs_, (f.size,)))
    return m, v


def ref_mix(spec, q):
    node = spec.mixture_rows
    K, N = node.K, node.y.size
    m, v = np.empty((len(q), N)), np.empty((len(q), N))
    for s, qs in enumerate(q):
        x = tl._constrained(spec, qs)
        mu = x[spec.vars[node.mu].offset :][:K]
        sigma = x[spec.vars[node.sigma].offset :][:K] if node.sigma is not None else np.broadcast_to(np.asarray(node.sigma_const, dtype="float64"), (K,))
        if node.w_logits is not None:
            e = x[spec.vars[node.w_logits].offset :][:K]
            w = np.exp(e - logsumexp(e))
        else:
            w = np.asarray(node.w_const, dtype="float64")
        m[s], v[s] = ref.mixture_moments(mu, sigma, w)
    return m, v


# ---- what every node is held to ------------------------------------------------------------------------------------------------
def _numpy_on_the_matrix(m, v, lp):
    """sums in extended precision, so that the reference's own rounding stays out of the 1e-12"""
    mw, vw = m.astype(np.longdouble), v.astype(np.longdouble)
    with np.errstate(all="ignore"):
        out = [mw.mean(0).astype("float64"), mw.var(0).astype("float64"), vw.mean(0).astype("float64")]
        lw = lp.astype(np.longdouble)
        top = lw.max(0)
        top = np.where(np.isfinite(top), top, 0.0)
        out.append((np.log(np.exp(lw - top).sum(0)) + top - np.log(np.longdouble(len(m)))).astype("float64"))
        second = (vw + mw * mw).mean(0)
        out.append((second - mw.mean(0) ** 2).astype("float64"))
        out.append(second.astype("float64"))
    return out


def _rel_hold(got, want, label, atol=0.0):
    fin = _same_pattern(got, want, label)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=atol, err_msg=label)


def _check_node(label, spec, name, S, m_ref, v_ref, monkeypatch, seed=61):
    """`spec` carries the new rows.  m_ref / v_ref: q -> the restatement's moments, in the node's evaluation order."""
    for k in tl.SCHED_VARS:
        monkeypatch.delenv(k, raising=False)
    node = next(nd for nd in ms.observed_nodes(spec) if nd[0] == name)
    q = tl._draws(spec, S, seed=seed)
    f = tl._vg(spec)
    try:
        mean, var = f.predict_moments(name, q, node=node[1:3])
        assert mean.shape == var.shape == (S, node[3])
        only_mean, none = f.predict_moments(name, q, node=node[1:3], var=False)
        assert none is None and np.array_equal(only_mean, mean, equal_nan=True)
        lp = f.log_likelihood(name, q, node=node[1:3])
        a1, a2 = f.pred_accumulator(name, node=node[1:3]), f.pred_accumulator(name, node=node[1:3])
        a3 = f.pred_accumulator(name, with_y=False, node=node[1:3])
        try:
            a1.update(q)
            cuts = sorted({0, S // 3, (2 * S + 2) // 3, S})
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                a2.update(q[lo:hi])
            a3.update(q)
            r1, r2, r3 = a1.read(), a2.read(), a3.read()
        finally:
            for a in (a1, a2, a3):
                a.close()
    finally:
        f.close()
    # 1. per-draw moments against the restatement
    want_m, want_v = m_ref(q), v_ref(q)
    _hold_values(mean, want_m, label + " mean")
    _hold_values(var, want_v, label + " var")
    # 2. accumulators against NumPy on the matrix the device returned
    assert r1[4] == r2[4] == r3[4] == S
    for u, w in zip(r1[:4], r2[:4]):
        assert np.array_equal(u, w, equal_nan=True), label + ": the state depends on how the draws were split"
    for u, w in zip(r1[:3], r3[:3]):
        assert np.array_equal(u, w, equal_nan=True), label + ": the moments depend on whether held-out values exist"
    assert r3[3] is None
    w_mean, w_vb, w_vw, w_lpd, w_total, w_second = _numpy_on_the_matrix(mean, var, lp)
    _rel_hold(r1[0], w_mean, label + " mean_i")
    _rel_hold(r1[1], w_vb, label + " var_between_i")
    _rel_hold(r1[2], w_vw, label + " var_within_i")
    _rel_hold(r1[3], w_lpd, label + " lpd_i", atol=1e-15)
    fin = _same_pattern(r1[1] + r1[2], w_total, label + " total variance")
    total = (r1[1] + r1[2])[fin]
    assert np.all(np.abs(total - w_total[fin]) <= 1e-12 * np.abs(w_total[fin]) + 1e-12 * w_second[fin]), label + " total variance"
    # 3. the same draws through batches of 1, 3 and 8: bit for bit
    for b in ("1", "3", "8"):
        monkeypatch.setenv("NUTS_LL_B", b)
        g = tl._vg(spec)
        try:
            mb, vb = g.predict_moments(name, q, node=node[1:3])
            parts = [g.predict_moments(name, q[lo:hi], node=node[1:3]) for lo, hi in zip(cuts[:-1], cuts[1:])]
        finally:
            g.close()
        assert np.array_equal(mb, mean, equal_nan=True) and np.array_equal(vb, var, equal_nan=True), (label, "NUTS_LL_B", b)
        assert np.array_equal(np.concatenate([p[0] for p in parts]), mean, equal_nan=True), (label, "split", b)
        assert np.array_equal(np.concatenate([p[1] for p in parts]), var, equal_nan=True), (label, "split", b)
    monkeypatch.delenv("NUTS_LL_B")
    return q, mean, var


# ---- 1. GLM node ------------------------------------------------------------------------------------------------------------------
def _glm_new(family, P, M, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(M, P)) * (0.5 / np.sqrt(P))
    y = rng.normal(size=M) if family == "normal" else (rng.random(M) < 0.5).astype("float64") if family == "bernoulli" else rng.poisson(2.0, size=M).astype("float64")
    return X, y


GLM_CASES = [("normal", 1, 1, 1), ("bernoulli", 1, 255, 8), ("poisson", 1, 256, 9), ("normal", 3, 257, 19), ("bernoulli", 3, 513, 8),
             ("poisson", 3, 1, 9), ("normal", 17, 255, 19), ("bernoulli", 17, 256, 1), ("poisson", 17, 513, 9)]


@pytest.mark.parametrize("family,P,M,S", GLM_CASES)
def test_glm_at_new_rows(family, P, M, S, monkeypatch):
    train = tl.glm_model(family, P, 40, True, "var", False)
    X, y = _glm_new(family, P, M, seed=70 + M)
    spec = with_data(train, {"y": {"X": X, "y": y}})
    _check_node(f"glm {family} P={P} M={M} S={S}", spec, "y", S, lambda q: ref_glm(spec, q)[0], lambda q: ref_glm(spec, q)[1], monkeypatch)


# ---- 2. logit rows ------------------------------------------------------------------------------------------------------------------
def _rows_new(D, M, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(M, D)) * (0.5 / np.sqrt(D))
    g = rng.choice([0, 2], size=M).astype("int32") if M > 1 else np.array([2], dtype="int32")    # G = 3: group 1 has no new row
    return X, (rng.random(M) < 0.5).astype("int8"), g


@pytest.mark.parametrize("D,M,S", [(1, 255, 9), (3, 257, 19), (8, 513, 8), (3, 1, 1), (8, 256, 9)])
def test_logit_rows_at_new_rows_unsorted_with_an_absent_group(D, M, S, monkeypatch):
    train = tl.rows_model([5, 4, 6], D, False)[0]
    X, y, g = _rows_new(D, M, seed=80 + M)
    spec = with_data(train, {"y": {"X": X, "group_idx": g, "y": y}})
    assert M == 1 or spec.rows_order is not None
    order = np.arange(M) if spec.rows_order is None else np.asarray(spec.rows_order)
    _check_node(f"rows D={D} M={M} S={S}", spec, "y", S, lambda q: ref_rows(spec, q, X, g)[0][:, order], lambda q: ref_rows(spec, q, X, g)[1][:, order], monkeypatch)


def test_unsorted_logit_rows_come_back_in_the_order_they_were_passed():
    train = tl.rows_model([5, 4, 6], 3, False)[0]
    X, y, g = _rows_new(3, 257, seed=81)
    q = tl._draws(train, 9, seed=82)
    out = predictive.predict(train, q[None], {"y": {"X": X, "group_idx": g, "y": y}}, expected=True, device=0)
    spec = with_data(train, {"y": {"X": X, "group_idx": g, "y": y}})
    m, v = ref_rows(spec, q, X, g)       # the caller's order
    _hold_values(out["expected"][0], m, "expected")
    np.testing.assert_allclose(out["mean"], m.mean(0), rtol=1e-10)
    np.testing.assert_allclose(out["var_within"], v.mean(0), rtol=1e-10)
    lp = tl.ref_rows(spec, q, X, y, g)
    np.testing.assert_allclose(out["lpd_i"], logsumexp(lp, axis=0) - np.log(9.0), **TOL)
    assert out["n_samples"] == 9 and out["n_data_points"] == 257 and out["elpd"] == float(out["lpd_i"].sum())
    # the same rows passed sorted: the same numbers, permuted
    o = np.argsort(g, kind="stable")
    again = predictive.predict(train, q[None], {"y": {"X": X[o], "group_idx": g[o], "y": y[o]}}, device=0)
    for k in ("mean", "var_between", "var_within", "lpd_i"):
        assert np.array_equal(again[k], out[k][o]), k


# ---- 3. element-wise factors -------------------------------------------------------------------------------------------------------
def _factor_data(N, seed):
    rng = np.random.default_rng(seed)
    return dict(loc=rng.normal(size=N), x1=rng.uniform(-1.0, 1.0, size=N), expo=rng.uniform(0.5, 2.0, size=N), x2=rng.uniform(-1.0, 1.0, size=N),
                x3=rng.uniform(-1.0, 1.0, size=N), y_normal=rng.normal(size=N), y_poisson=rng.poisson(1.5, size=N).astype("float64"),
                y_binomial=rng.integers(0, 11, size=N).astype("float64"), y_studentt=rng.normal(size=N))


def factor_model(d):
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    b = m.Normal("b", 0.0, 1.0)
    s = m.HalfNormal("s", 1.0)
    m.Normal("y_normal", a + m.as_expr(d["loc"]), s, observed=d["y_normal"])
    m.Poisson("y_poisson", m.as_expr(d["expo"]) * m.math.exp(a + b * m.as_expr(d["x1"])), observed=d["y_poisson"])
    m.Binomial("y_binomial", 10.0, m.math.sigmoid(a + b * m.as_expr(d["x2"])), observed=d["y_binomial"])
    m.StudentT("y_studentt", 1.5, a + b * m.as_expr(d["x3"]), s, observed=d["y_studentt"])
    return m.build()


FACTOR_INPUTS = {"y_normal": ("loc",), "y_poisson": ("expo", "x1"), "y_binomial": ("x2",), "y_studentt": ("x3",)}


def _factor_new(train, name, d):
    ids = data_inputs(train)[name]["data"]
    assert len(ids) == len(FACTOR_INPUTS[name])
    return {name: {"data": {i: d[k] for i, k in zip(ids, FACTOR_INPUTS[name])}, "observed": d[name]}}


@pytest.mark.parametrize("name,M,S", [("y_normal", 255, 9), ("y_normal", 1, 1), ("y_poisson", 257, 19), ("y_poisson", 256, 8), ("y_binomial", 513, 9),
                                      ("y_binomial", 255, 1), ("y_studentt", 257, 8), ("y_studentt", 513, 19)])
def test_factors_at_new_rows(name, M, S, monkeypatch):
    train = factor_model(_factor_data(40, seed=90))
    d = _factor_data(M, seed=91 + M)
    spec = with_data(train, _factor_new(train, name, d))
    fresh = factor_model({k: (d[k] if k in FACTOR_INPUTS[name] + (name,) else v) for k, v in _factor_data(40, seed=90).items()})
    fi = next(nd[2] for nd in ms.observed_nodes(spec) if nd[0] == name)
    assert spec.factors[fi].size == M and np.array_equal(spec.data[spec.factors[fi].args[0].a.ref], fresh.data[fresh.factors[fi].args[0].a.ref])
    q, mean, var = _check_node(f"{name} M={M} S={S}", spec, name, S, lambda q: ref_factor(spec, fi, q)[0], lambda q: ref_factor(spec, fi, q)[1], monkeypatch)
    if name == "y_studentt":
        assert np.all(var == np.inf) and np.all(np.isfinite(mean)), "nu = 1.5: the infinite variance must arrive as +inf"
    # the held-out log-density is the pointwise log-likelihood of the oracle
    out = predictive.predict(train, q[None], _factor_new(train, name, d), var_name=name, device=0)
    np.testing.assert_allclose(out["lpd_i"], logsumexp(tl.ref_factor(spec, fi, q), axis=0) - np.log(float(S)), **TOL)
    if name == "y_studentt":
        assert np.all(out["var_within"] == np.inf) and np.all(out["sd"] == np.inf) and np.all(np.isfinite(out["var_between"]))


def test_a_check_killed_draw_has_nan_moments_and_no_weight_in_the_lpd():
    rng = np.random.default_rng(95)
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0)
    s = m.HalfNormal("s", 1.0, transform=None)       # untransformed: a draw may be negative
    m.Normal("y", mu + m.as_expr(rng.normal(size=6)), m.math.check(m.math.abs(s), m.math.gt(s, 0.0)), observed=rng.normal(size=6))
    train = m.build()
    (loc_id,) = data_inputs(train)["y"]["data"]
    loc, y = rng.normal(size=9), rng.normal(size=9)
    new = {"y": {"data": {loc_id: loc}, "observed": y}}
    spec = with_data(train, new)
    q = np.array([[0.1, 0.8], [0.2, -0.3], [-0.4, 1.2], [0.3, -1.0], [0.0, 0.5]])
    dead = np.array([False, True, False, True, False])
    f = tl._vg(spec)
    try:
        mean, var = f.predict_moments("y", q)
        lp = f.log_likelihood("y", q)
    finally:
        f.close()
    assert np.all(np.isnan(mean[dead])) and np.all(np.isnan(var[dead])) and np.all(np.isneginf(lp[dead]))
    np.testing.assert_allclose(mean[~dead], q[~dead, :1] + loc[None, :], **TOL)
    np.testing.assert_allclose(var[~dead], np.broadcast_to(q[~dead, 1:] ** 2, (3, 9)), **TOL)
    # folded: the NaN moments are not hidden; in the lpd the dead draws weigh nothing and the count is still all five
    out = predictive.predict(train, q[None], new, device=0)
    assert np.all(np.isnan(out["mean"])) and np.all(np.isnan(out["var_within"])) and out["n_samples"] == 5
    np.testing.assert_allclose(out["lpd_i"], logsumexp(lp[~dead], axis=0) - np.log(5.0), rtol=1e-12)
    alive = predictive.predict(train, q[~dead][None], new, device=0)
    np.testing.assert_allclose(alive["mean"], mean[~dead].mean(0), rtol=1e-12)
    np.testing.assert_allclose(alive["lpd_i"], out["lpd_i"] + np.log(5.0 / 3.0), rtol=1e-12)
    # nothing but dead draws: lpd = -inf, never NaN
    none = predictive.predict(train, q[dead][None], new, device=0)
    assert np.all(np.isneginf(none["lpd_i"])) and none["elpd"] == -np.inf


# ---- 4. marginal mixture ---------------------------------------------------------------------------------------------------------
def mix_model(K, y, seed=96):
    m = ModelBuilder()
    w = ("softmax", m.Normal("logits", 0.0, 1.0, shape=K))
    mu = m.Normal("mu", 0.0, 10.0, shape=K)
    sigma = m.HalfNormal("sigma", 2.0, shape=K)
    m.NormalMixture("y", w, mu, sigma, y)
    return m.build()


@pytest.mark.parametrize("K,M,S", [(2, 257, 9), (16, 513, 19), (16, 1, 8)])
def test_marginal_mixture_at_new_rows(K, M, S, monkeypatch):
    rng = np.random.default_rng(97)
    train = mix_model(K, rng.normal(size=50) * 2.0)
    y = rng.normal(size=M) * 2.0
    spec = with_data(train, {"y": {"y": y}})
    q, mean, var = _check_node(f"mixture K={K} M={M} S={S}", spec, "y", S, lambda q: ref_mix(spec, q)[0], lambda q: ref_mix(spec, q)[1], monkeypatch)
    out = predictive.predict(train, q[None], {"y": {"y": y}}, device=0)
    np.testing.assert_allclose(out["lpd_i"], logsumexp(tl.ref_mix(spec, q), axis=0) - np.log(float(S)), **TOL)


# ---- 5. at the training data ------------------------------------------------------------------------------------------------------
def _training_cases():
    spec = tl.glm_model("poisson", 9, 300, True, None, False)
    yield "glm poisson", spec, "y", {"y": {"X": spec.glm_rows.X, "y": spec.glm_rows.y}}
    spec = tl.glm_model("normal", 17, 257, True, "var", False)
    yield "glm normal", spec, "y", {"y": {"X": spec.glm_rows.X, "y": spec.glm_rows.y}}
    spec, X, y, g = tl.rows_model(tl.RAGGED, 3, False)
    yield "rows", spec, "y", {"y": {"X": X, "group_idx": g, "y": y}}
    d = _factor_data(257, seed=98)
    spec = factor_model(d)
    yield "factor", spec, "y_poisson", _factor_new(spec, "y_poisson", d)
    spec = tl.mix_model("softmax")
    yield "mixture", spec, "y", {"y": {"y": spec.mixture_rows.y}}


def test_at_the_training_data_predict_is_waic_lppd_and_the_fitted_models_moments():
    for label, spec, name, new in _training_cases():
        q = tl._draws(spec, 2 * 9, seed=99).reshape(2, 9, spec.n)
        out = predictive.predict(spec, q, new, var_name=name, expected=True, device=0)
        waic = loglik.waic(spec, q, var_name=name, pointwise=True, device=0)
        print(label, "max abs difference lpd_i - lppd_i", float(np.abs(out["lpd_i"] - waic["lppd_i"]).max()))
        np.testing.assert_allclose(out["lpd_i"], waic["lppd_i"], rtol=1e-10, atol=0, err_msg=label)
        node = next(nd for nd in ms.observed_nodes(spec) if nd[0] == name)
        f = tl._vg(spec)
        try:
            own = loglik.caller_order(spec, node[1], f.predict_moments(name, q.reshape(18, -1), node=node[1:3], var=False)[0])
        finally:
            f.close()
        assert np.array_equal(out["expected"].reshape(18, -1), own), label
        assert out["n_samples"] == 18 and out["expected"].shape[:2] == (2, 9)


# ---- 6. replicates at new rows -------------------------------------------------------------------------------------------------------
def test_replicates_at_the_training_rows_are_those_of_the_fitted_model():
    for label, spec, name, new in _training_cases():
        q = tl._draws(spec, 2 * 9, seed=100).reshape(2, 9, spec.n)
        out = predictive.predict(spec, q, new, var_name=name, replicates=True, random_seed=SEED, chain_ids=[3, 1], device=0)
        want = predictive.sample_posterior_predictive(spec, q, var_names=[name], random_seed=SEED, chain_ids=[3, 1], device=0)[name]
        assert np.array_equal(out["predictions"], want, equal_nan=True), label


def test_replicates_at_other_rows_against_the_restatement():
    S = 9
    train = tl.glm_model("poisson", 3, 40, True, None, False)
    X, y = _glm_new("poisson", 3, 257, seed=101)
    q = tl._draws(train, S, seed=102)
    out = predictive.predict(train, q[None], {"y": {"X": X}}, replicates=True, random_seed=SEED, device=0)
    assert "lpd_i" not in out and "elpd" not in out
    want, margin, discrete = tp.ref_glm(with_data(train, {"y": {"X": X}}), q, SEED)
    tp._hold("glm poisson", out["predictions"][0], want, margin, discrete)
    train = tl.glm_model("bernoulli", 17, 40, True, None, False)
    X, y = _glm_new("bernoulli", 17, 255, seed=103)
    q = tl._draws(train, S, seed=104)
    out = predictive.predict(train, q[None], {"y": {"X": X, "y": y}}, replicates=True, random_seed=SEED, device=0)
    want, margin, discrete = tp.ref_glm(with_data(train, {"y": {"X": X, "y": y}}), q, SEED)
    tp._hold("glm bernoulli", out["predictions"][0], want, margin, discrete)
    train = tl.rows_model([5, 4, 6], 3, False)[0]
    X, y, g = _rows_new(3, 257, seed=105)
    q = tl._draws(train, S, seed=106)
    new = {"y": {"X": X, "group_idx": g}}
    out = predictive.predict(train, q[None], new, replicates=True, random_seed=SEED, device=0)
    spec = with_data(train, new)
    want, margin = tp.ref_rows(spec, q, X, g, SEED)      # the spec's sorted order
    back = lambda a: loglik.caller_order(spec, ms.LL_LOGIT_ROWS, a)   # noqa: E731
    tp._hold("rows", out["predictions"][0], back(want), back(margin), True)
    d = _factor_data(257, seed=107)
    train = factor_model(_factor_data(40, seed=90))
    q = tl._draws(train, S, seed=108)
    new = _factor_new(train, "y_normal", d)
    out = predictive.predict(train, q[None], new, var_name="y_normal", replicates=True, random_seed=SEED, device=0)
    spec = with_data(train, new)
    fi = next(nd[2] for nd in ms.observed_nodes(spec) if nd[0] == "y_normal")
    want, margin = tp.ref_factor(spec, fi, q, SEED)
    tp._hold("factor normal", out["predictions"][0], want, margin, False)
    with pytest.raises(ValueError, match="Binomial"):
        predictive.predict(train, q[None], _factor_new(train, "y_binomial", d), var_name="y_binomial", replicates=True, device=0)


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------
def test_sample_then_predict_at_held_out_rows():
    from pymc_amd.sampling import sample

    G, D = 8, 8
    spec = models.hier_logit(G=G, rows_per_group=20)
    Xh, yh, gh = models._hier_logit_data(G, D, 5, seed=4242)
    perm = np.random.default_rng(110).permutation(len(yh))
    Xh, yh, gh = Xh[perm], yh[perm], gh[perm]
    res = sample(draws=200, tune=200, chains=2, model=spec, random_seed=109, device=0)
    try:
        out = predictive.predict(spec, res, {"y": {"X": Xh, "group_idx": gh, "y": yh}}, device=0)
        bare = predictive.predict(spec, res, {"y": {"X": Xh, "group_idx": gh}}, device=0)
    finally:
        res["step"].close()
    assert out["n_samples"] == 400 and out["n_data_points"] == len(yh)
    assert np.isfinite(out["elpd"]) and np.isfinite(out["se"]) and np.all(np.isfinite(out["lpd_i"])) and np.all(out["lpd_i"] < 0.0)
    assert np.all((out["mean"] > 0.0) & (out["mean"] < 1.0))
    # an identity of the Bernoulli mixture: its variance is mean (1 - mean), whatever the draws
    np.testing.assert_allclose(out["sd"] ** 2, out["mean"] * (1.0 - out["mean"]), rtol=1e-12)
    # lpd_i of a Bernoulli observation is the log of the predicted probability of what was observed
    np.testing.assert_allclose(out["lpd_i"], np.log(np.where(yh != 0, out["mean"], 1.0 - out["mean"])), rtol=1e-10)
    assert "lpd_i" not in bare and all(np.array_equal(bare[k], out[k]) for k in ("mean", "var_between", "var_within", "sd"))
