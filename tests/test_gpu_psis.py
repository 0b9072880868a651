"""Streaming PSIS-LOO on the device (csrc/psis.h, k_psis_fold / k_psis_finish, `nuts_psis_*`, `loglik.loo`).

Reference: the NumPy restatement of the published algorithm (tests/psis_reference.py, `psis_direct`: the whole vector per
observation) applied to the device's OWN [S][N] values from `compute_log_likelihood` -- that path is held to the oracle at 1e-10 by
tests/test_gpu_loglik.py, and a draw's values do not depend on its batch (tested there, bit for bit), so the state sees exactly the
values the reference gets and the comparison isolates the new arithmetic.

Bars: elpd_loo_i and every finite khat rtol = atol = 1e-9 (the project's WAIC bar); infinities and NaNs in the same places;
lppd_i within 1e-12 of `nuts_waic_read`'s.

Draws are random positions N(0, scale^2), not a sampled chain; the scale of each model is chosen so that at S = 203 the reference's
khat falls below 0.3 at some observation and above 0.7 at another (asserted on the reference before anything is compared; a model
with ONE observation has one khat and is exempt).  Each model's trace of 203 draws is evaluated once; S = 20, 21, 37, 203 are its
prefixes: S = 20 has M = 4 (no tail is ever fitted: khat = +inf everywhere, asserted), S = 21 the smallest fit (5 values), and none
of them is a multiple of the batch of 8.

With PYMC_AMD_PSIS_JSON set to a path, the run writes the measured maxima there (profiles/psis_loo.json).
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psis_reference as pr  # noqa: E402
from test_gpu_loglik import factor_model, glm_model, mix_model, rows_model  # noqa: E402

from pymc_amd import loglik, models  # noqa: E402
from pymc_amd import model_spec as ms  # noqa: E402
from pymc_amd.model_spec import ModelBuilder  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-9, atol=1e-9)
S_ALL = 203
S_LIST = [20, 21, 37, 203]
MEASURED = {}

# label -> (spec builder, observed variable, scale of the draws, seed)
MODELS = {
    "factor_1": (lambda: factor_model(1), "y_studentt", 0.5, 1),
    "factor_257": (lambda: factor_model(257), "y_studentt", 0.5, 1),
    "glm_1000x3": (lambda: glm_model("bernoulli", 3, 1000, True, None, False), "y", 1.0, 2),
    "rows_unequal_groups": (lambda: rows_model([1, 70, 129, 33], 3, False)[0], "y", 0.75, 3),
    "mixture": (lambda: mix_model("dirichlet"), "y", 0.5, 4),
}


def _vg(spec):
    from pymc_amd.value_grad import DeviceValueGradFunction

    return DeviceValueGradFunction(spec, device=0)


class Trace:
    """One model, its 203 draws and the device's own values of them (caller's order), evaluated once and left unchanged."""

    def __init__(self, label):
        build, self.name, scale, seed = MODELS[label]
        self.label = label
        self.spec = build()
        self.q = np.random.default_rng(seed).normal(size=(S_ALL, self.spec.n)) * scale
        self.f = _vg(self.spec)
        self.ll = loglik.compute_log_likelihood(self.spec, self.q[None], var_names=[self.name], func=self.f)[self.name][0]
        self.ll.setflags(write=False)
        self._ref = {}

    def ref(self, S):
        if S not in self._ref:
            self._ref[S] = pr.psis_matrix(self.ll[:S])
        return self._ref[S]


@pytest.fixture(scope="module")
def traces():
    made = {}

    def get(label):
        if label not in made:
            made[label] = Trace(label)
        return made[label]

    yield get
    for t in made.values():
        t.f.close()
    path = os.environ.get("PYMC_AMD_PSIS_JSON")
    if path and MEASURED:
        with open(path, "w") as fh:
            json.dump(MEASURED, fh, indent=1, sort_keys=True)


def _compare(label, got, ref, S):
    """got = loo(..., pointwise=True); ref = (khat, elpd_i, lppd_i) of the restatement"""
    khat, elpd_i, lppd_i = ref
    fin = np.isfinite(khat)
    assert np.array_equal(np.isfinite(got["pareto_k"]), fin) and np.array_equal(np.isnan(got["pareto_k"]), np.isnan(khat))
    assert np.array_equal(got["pareto_k"][~fin & ~np.isnan(khat)], khat[~fin & ~np.isnan(khat)])
    efin = np.isfinite(elpd_i)
    assert np.array_equal(np.isfinite(got["loo_i"]), efin) and np.array_equal(np.isnan(got["loo_i"]), np.isnan(elpd_i))
    assert np.array_equal(got["loo_i"][~efin & ~np.isnan(elpd_i)], elpd_i[~efin & ~np.isnan(elpd_i)])
    dk = float(np.abs(got["pareto_k"][fin] - khat[fin]).max()) if fin.any() else 0.0
    de = float((np.abs(got["loo_i"][efin] - elpd_i[efin]) / np.maximum(1.0, np.abs(elpd_i[efin]))).max()) if efin.any() else 0.0
    print(label, "S", S, "max |khat - ref|", dk, "max rel |elpd_loo_i - ref|", de)
    MEASURED[f"{label}/S={S}"] = {"khat_abs": dk, "elpd_loo_i_rel": de}
    np.testing.assert_allclose(got["pareto_k"][fin], khat[fin], **TOL)
    np.testing.assert_allclose(got["loo_i"][efin], elpd_i[efin], **TOL)
    summ = pr.loo_summary(khat, elpd_i, lppd_i, S)
    assert got["warning"] == summ["warning"] and got["good_k"] == summ["good_k"]
    assert got["n_samples"] == S and got["n_data_points"] == khat.size
    if efin.all():
        np.testing.assert_allclose([got["elpd_loo"], got["se"], got["p_loo"]], [summ["elpd_loo"], summ["se"], summ["p_loo"]], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("S", S_LIST)
@pytest.mark.parametrize("label", list(MODELS))
def test_loo_against_the_restatement_on_the_devices_own_values(label, S, traces):
    t = traces(label)
    khat203 = t.ref(S_ALL)[0]
    if khat203.size > 1:
        assert khat203.min() < 0.3 and khat203[np.isfinite(khat203)].max() > 0.7, (khat203.min(), khat203.max())
    khat, elpd_i, lppd_i = t.ref(S)
    assert np.all(np.isfinite(elpd_i))
    if S == 20:
        assert np.all(khat == np.inf)                # M = 4: a tail of at most 4 values is never fitted
    if S == 21:
        assert np.all(np.isfinite(khat))             # the smallest fit: 5 values
    got = loglik.loo(t.spec, t.q[None, :S], var_name=t.name, pointwise=True, func=t.f)
    _compare(label, got, (khat, elpd_i, lppd_i), S)
    if S == S_ALL and khat.size > 1:
        assert got["warning"] is True


def test_lppd_is_the_waic_accumulators(traces):
    t = traces("glm_1000x3")
    w = t.f.waic_accumulator(t.name)
    p = t.f.psis_accumulator(t.name, S_ALL)
    try:
        w.update(t.q)
        p.update(t.q)
        lppd_w, _, n = w.read()
        elpd, khat, lppd_p, n2 = p.read()
    finally:
        w.close()
        p.close()
    assert n == n2 == S_ALL
    np.testing.assert_allclose(lppd_p, lppd_w, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lppd_p, t.ref(S_ALL)[2], rtol=1e-12, atol=1e-12)


def test_the_state_does_not_depend_on_how_the_draws_were_split(traces):
    t = traces("glm_1000x3")
    raws = []
    for split in ([S_ALL], [5, 8, 190], [1] * S_ALL):
        p = t.f.psis_accumulator(t.name, S_ALL)
        try:
            s0 = 0
            for k in split:
                p.update(t.q[s0:s0 + k])
                s0 += k
            raws.append(p.raw())
        finally:
            p.close()
    keep, acc, n = raws[0]
    assert n == S_ALL and keep.shape == (pr.tail_len(S_ALL) + 1, 1000) and acc.shape == (4, 1000)
    for other in raws[1:]:
        assert other[2] == S_ALL
        assert np.array_equal(keep, other[0]) and np.array_equal(acc, other[1]), "the state depends on how the draws were split"
    # and it is what the restatement keeps: the M + 1 smallest values of each observation, ascending
    assert np.array_equal(keep, np.sort(t.ll, axis=0)[:keep.shape[0]])
    k0, m0, r0 = pr.fold(t.ll[:, 17])
    assert np.array_equal(keep[:, 17], k0) and acc[2, 17] == m0
    np.testing.assert_allclose(acc[3, 17], r0, rtol=1e-13)


def test_duplicated_draws_tie_at_the_cutoff(traces):
    """The second half of the trace repeats the first: every value occurs twice, the cutoff is tied with a tail value or with the
    value below it at every observation."""
    t = traces("factor_257")
    half = 100
    q = np.concatenate([t.q[:half], t.q[:half]])
    ll = np.concatenate([t.ll[:half], t.ll[:half]])
    ref = pr.psis_matrix(ll)
    M = pr.tail_len(2 * half)
    srt = np.sort(ll, axis=0)
    assert np.all((srt[M] == srt[M - 1]) | (srt[M] == srt[M + 1]))
    got = loglik.loo(t.spec, q[None], var_name=t.name, pointwise=True, func=t.f)
    _compare("factor_257 duplicated", got, ref, 2 * half)


def test_minus_infinity_at_some_draws():
    """A failed parameter check (an untransformed scale below 0) kills factor `y` at that draw: khat = +inf and elpd_loo_i = -inf at
    each of its observations; `y2`, which does not read the scale, stays finite at all of them."""
    rng = np.random.default_rng(5)
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0)
    s = m.HalfNormal("s", 1.0, transform=None)       # untransformed: a draw may be negative
    m.Normal("y", mu, s, observed=rng.normal(size=7))
    m.Normal("y2", mu, 1.0, observed=rng.normal(size=9))
    spec = m.build()
    S = 37
    q = np.column_stack([rng.normal(size=S) * 0.5, 0.5 + rng.random(S)])
    q[11, 1] = -0.3
    q[30, 1] = -0.1
    f = _vg(spec)
    try:
        ll = loglik.compute_log_likelihood(spec, q[None], func=f)
        assert np.all(np.isneginf(ll["y"][0][[11, 30]])) and np.isfinite(np.delete(ll["y"][0], [11, 30], axis=0)).all()
        got = loglik.loo(spec, q[None], var_name="y", pointwise=True, func=f)
        assert np.all(got["pareto_k"] == np.inf) and np.all(got["loo_i"] == -np.inf) and got["warning"] is True
        ref = pr.psis_matrix(ll["y"][0])
        assert np.array_equal(got["pareto_k"], ref[0]) and np.array_equal(got["loo_i"], ref[1])
        got2 = loglik.loo(spec, q[None], var_name="y2", pointwise=True, func=f)
        assert np.all(np.isfinite(got2["pareto_k"])) and np.all(np.isfinite(got2["loo_i"]))
        _compare("minus_inf/y2", got2, pr.psis_matrix(ll["y2"][0]), S)
        # -inf at one observation only (outside the support at some draws): finite at the others of the same factor
        m = ModelBuilder()
        t = m.Normal("t", 0.0, 1.0)
        m.spec.data.append(np.array([0.1, 3.0, 4.0]))
        value = ms.Term(ms.Operand(ms.OP_DATA, 0.0, len(m.spec.data) - 1), ms.Operand(ms.OP_CONST, -1.0), t.term.a)
        m.spec.factors.append(ms.Factor(ms.D_HALFNORMAL, 3, (value, ms.Term(ms.Operand(ms.OP_CONST, 1.0))), 0.0, "y", (), observed=True))
        spec3 = m.build()
        q3 = rng.normal(size=(S, 1)) * 0.5
        q3[3, 0] = 0.4
        g = _vg(spec3)
        try:
            ll3 = loglik.compute_log_likelihood(spec3, q3[None], func=g)["y"][0]
            assert np.any(np.isneginf(ll3[:, 0])) and np.all(np.isfinite(ll3[:, 1:]))
            got3 = loglik.loo(spec3, q3[None], pointwise=True, func=g)
            assert got3["pareto_k"][0] == np.inf and got3["loo_i"][0] == -np.inf
            assert np.all(np.isfinite(got3["pareto_k"][1:])) and np.all(np.isfinite(got3["loo_i"][1:]))
            _compare("minus_inf/support", got3, pr.psis_matrix(ll3), S)
        finally:
            g.close()
    finally:
        f.close()


def test_two_chains_pooled_are_the_concatenated_trace(traces):
    t = traces("rows_unequal_groups")
    one = loglik.loo(t.spec, t.q[None, :202], var_name=t.name, pointwise=True, func=t.f)
    two = loglik.loo(t.spec, t.q[:202].reshape(2, 101, -1), var_name=t.name, pointwise=True, func=t.f)
    assert one["n_samples"] == two["n_samples"] == 202
    for k in one:
        assert np.array_equal(one[k], two[k]), k
    # results are in the CALLER's row order: the rows were passed unsorted
    assert t.spec.rows_order is not None
    _compare("rows pooled", two, pr.psis_matrix(t.ll[:202]), 202)


def test_misuse_is_an_error_with_a_text(traces):
    t = traces("factor_257")
    p = t.f.psis_accumulator(t.name, 21)
    try:
        p.update(t.q[:13])
        with pytest.raises(ValueError, match="13 of 21 draws"):
            p.read()
        with pytest.raises(ValueError, match="exceed the 21"):
            p.update(t.q[:9])
        keep, acc, n = p.raw()          # (refused calls changed nothing)
        assert n == 13 and keep.shape == (6, 257) and np.all(np.isfinite(keep))
        p.update(t.q[13:21])
        elpd, khat, lppd, n = p.read()
        assert n == 21
        ref = t.ref(21)
        np.testing.assert_allclose(elpd, ref[1], **TOL)
        np.testing.assert_allclose(khat, ref[0], **TOL)
    finally:
        p.close()
    with pytest.raises(ValueError, match="cap of 1024"):
        t.f.psis_accumulator(t.name, 200000)
    t.f.psis_accumulator(t.name, 116000).close()          # K1 = 1023: under the cap
    with pytest.raises(ValueError, match="at least 2"):
        t.f.psis_accumulator(t.name, 1)
    with pytest.raises(ValueError, match="reff"):
        t.f.psis_accumulator(t.name, 100, reff=0.0)
    # a relative efficiency below 1 lengthens the tail: M = ceil(min(S / 5, 3 sqrt(S / reff)))
    got = loglik.loo(t.spec, t.q[None], var_name=t.name, pointwise=True, reff=0.3, func=t.f)
    assert pr.tail_len(S_ALL, 0.3) == 41 and pr.tail_len(1000, 0.5) == 135
    _compare("factor_257 reff 0.3", got, pr.psis_matrix(t.ll, 0.3), S_ALL)


def test_reff_changes_the_tail_length():
    spec = factor_model(257)
    q = np.random.default_rng(6).normal(size=(1000, spec.n)) * 0.5
    f = _vg(spec)
    try:
        ll = f.log_likelihood("y_studentt", q)
        p = f.psis_accumulator("y_studentt", 1000, reff=0.5)
        try:
            p.update(q)
            keep, _, _ = p.raw()
            elpd, khat, _, _ = p.read()
        finally:
            p.close()
    finally:
        f.close()
    assert keep.shape[0] == 136 != pr.tail_len(1000) + 1
    ref = pr.psis_matrix(ll, 0.5)
    got = {"pareto_k": khat, "loo_i": elpd}
    fin = np.isfinite(ref[0])
    assert fin.all()
    print("S 1000 reff 0.5: max |khat - ref|", np.abs(khat - ref[0]).max(), "max |elpd - ref|", np.abs(elpd - ref[1]).max())
    MEASURED["factor_257 reff 0.5/S=1000"] = {"khat_abs": float(np.abs(khat - ref[0]).max()),
                                              "elpd_loo_i_rel": float((np.abs(elpd - ref[1]) / np.maximum(1.0, np.abs(ref[1]))).max())}
    np.testing.assert_allclose(got["pareto_k"], ref[0], **TOL)
    np.testing.assert_allclose(got["loo_i"], ref[1], **TOL)


def test_chain_group_member_is_refused():
    from pymc_amd.chain_group import ChainGroup
    from pymc_amd.sampling import init_nuts

    spec = models.mvnormal(n=256, seed=5)
    step = init_nuts(spec, init="adapt_diag", chains=1, random_seed_list=[1], device=0, tune=10)[1]
    group = ChainGroup([step])
    try:
        with pytest.raises(ValueError, match="chain group"):
            step._logp_dlogp_func.psis_accumulator("x", 50, node=(ms.LL_FACTOR, 0))
    finally:
        group.close()
        step.close()
