"""Power-scaling sensitivity on the device (csrc/psens.h, csrc/psens_kernel.h; `nuts_model_logdens_sum`, `nuts_psens_weights`,
`nuts_psens`; pymc_amd/sensitivity.py).

References: tests/psens_reference.py (NumPy, and the same D at 200 bits: the truth), tests/psis_reference.py for the smoothing.

Bars
  * D = cjs^2 of `nuts_psens` (compared on D: the square root turns 1e-16 at D ~ 0 into 1e-8): the NumPy restatement's worst
    absolute error against the 200-bit truth over this file's inputs at S <= 1000 is MEASURED (`ref_err`), the device gets 8 x that
    -- a different but legitimate order of summation can differ by as much --, at S > 1000 against the restatement under the same
    bound x S / 1000.  Both numbers go to the file named by PYMC_AMD_PSENS_JSON.
  * rows of `nuts_psens`: bitwise across P, NUTS_PSENS_BLOCK, neighbours, and a permutation of the draws with their weights.
  * weights and khat of `nuts_psens_weights`: rtol = atol = 1e-9, the bar of tests/test_gpu_psis.py (atol / S for the weights, which
    are of order 1 / S); sum w = 1 within S eps.
  * `nuts_model_logdens_sum`: the row sums of `nuts_model_loglik` within N eps sum |terms| (counted: N - 1 additions, each rounding at
    most eps / 2 of a partial sum that never exceeds sum |terms|, in either order); bitwise across NUTS_LL_B, splits and company; exact
    on dyadic terms.
"""
import json
import math
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psens_reference as ps  # noqa: E402
import psis_reference as pr  # noqa: E402
from test_gpu_loglik import SCHED_VARS, factor_model, glm_model, rows_model  # noqa: E402

from pymc_amd import models, sensitivity  # noqa: E402
from pymc_amd import model_spec as ms  # noqa: E402
from pymc_amd.model_spec import ModelBuilder  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo("float64").eps
S_LIST = [2, 3, 255, 256, 257, 1000, 4096, 8192]
P_ALL = 70
COL_TIES, COL_CONST, COL_INF = 5, 6, 7
MEASURED = {}


def _vg(spec):
    from pymc_amd.value_grad import DeviceValueGradFunction

    return DeviceValueGradFunction(spec, device=0)


# ---- nuts_psens on synthetic arrays -------------------------------------------------------------------------------------------------------
class Synthetic:
    """S draws of 70 parameters, a component's log-density and the restatement's weights for both alphas; evaluated once."""

    def __init__(self, S):
        rng = np.random.default_rng(1000 + S)
        x = rng.standard_normal((S, P_ALL)) * np.exp(rng.standard_normal(P_ALL))
        x[:, COL_TIES] = rng.integers(0, 1000, size=S) % 7
        if S == 2:
            x[:, COL_TIES] = [3.0, 1.0]
        x[:, COL_CONST] = 2.5
        self.lc = -1.5 * (x[:, 0] / np.abs(x[:, 0]).max() - 0.3) ** 2 * S ** 0.5 + 0.5 * x[:, 1] / np.abs(x[:, 1]).max() + 0.05 * rng.standard_normal(S)
        x[S // 2, COL_INF] = np.inf
        self.S, self.x = S, x
        a_lo, a_hi = ps.alphas()
        self.w_lo, self.w_hi = ps.weights(self.lc, a_lo)[0], ps.weights(self.lc, a_hi)[0]
        for a in (self.x, self.lc, self.w_lo, self.w_hi):
            a.setflags(write=False)
        self._ref = None

    def ref(self):
        """[P][2]: D_lo, D_hi of the restatement"""
        if self._ref is None:
            self._ref = np.array([ps.psens_one(self.x[:, p], self.w_lo, self.w_hi)[:2] for p in range(P_ALL)])
        return self._ref


@pytest.fixture(scope="module")
def synth():
    made = {}

    def get(S):
        if S not in made:
            made[S] = Synthetic(S)
        return made[S]

    return get


MP_COLS = (0, 1, 2, COL_TIES)


@pytest.fixture(scope="module")
def ref_err(synth):
    """The restatement's worst |D - truth| over the inputs of this file at S <= 1000 (the columns MP_COLS of each S under both
    sets of weights and both signs, and the one-hot weights), measured once."""
    worst = 0.0
    for S in [s for s in S_LIST if s <= 1000]:
        t = synth(S)
        hot = _one_hot(t)
        for p in MP_COLS:
            for w in (t.w_lo, t.w_hi) + hot:
                for sign in (1.0, -1.0):
                    d, truth = ps.distance(sign * t.x[:, p], w), ps.distance_mp(sign * t.x[:, p], w)
                    worst = max(worst, abs(d - truth))
    MEASURED["reference_worst_abs_error_in_D"] = worst
    MEASURED["device_bound_in_D"] = 8.0 * worst
    print("restatement against the 200-bit truth: worst |D - truth|", worst, "-> the device's bound", 8.0 * worst)
    assert 0.0 < worst < 1e-13
    yield worst
    path = os.environ.get("PYMC_AMD_PSENS_JSON")
    if path:
        MEASURED["command"] = "PYMC_AMD_PSENS_JSON=profiles/psens_edges.json python -m pytest tests/test_gpu_psens.py -m gpu -q"
        with open(path, "w") as fh:
            json.dump(MEASURED, fh, indent=1, sort_keys=True)


def _one_hot(t):
    hot, other = np.zeros(t.S), np.zeros(t.S)
    hot[int(np.argmax(t.x[:, 0]))] = 1.0
    other[t.S // 3] = 1.0
    return hot, other


def _call(x, w_lo, w_hi, delta=0.01):
    out = sensitivity.psens_from_weights(x, w_lo, w_hi, delta, device=0)
    return np.stack([out[c] for c in sensitivity.COLUMNS])


def _hold(label, got, ref, bound):
    """got [3][P] of the device, ref [P][2] D of a reference: NaN in the same places, |cjs^2 - D| <= bound"""
    worst = 0.0
    for k in (0, 1):
        nan = np.isnan(ref[:, k])
        assert np.array_equal(np.isnan(got[k]), nan), (label, k)
        err = np.abs(got[k][~nan] ** 2 - ref[~nan, k])
        worst = max(worst, float(err.max()) if err.size else 0.0)
    print(label, "worst |D - ref|", worst, "bound", bound)
    MEASURED[label] = {"worst_abs_error_in_D": worst, "bound": bound}
    assert worst <= bound, (label, worst, bound)
    with np.errstate(invalid="ignore"):
        sens = (got[0] + got[1]) / (2.0 * math.log2(1.01))
    assert np.array_equal(np.isnan(got[2]), np.isnan(sens)) and np.allclose(got[2], sens, rtol=4 * EPS, atol=0.0, equal_nan=True), label


@pytest.mark.parametrize("S", S_LIST)
def test_distances_against_the_restatement_and_the_truth(S, synth, ref_err):
    t = synth(S)
    got = _call(t.x, t.w_lo, t.w_hi)
    assert np.all(np.isnan(got[:, COL_CONST])) and np.all(np.isnan(got[:, COL_INF]))
    fin = [p for p in range(P_ALL) if p not in (COL_CONST, COL_INF)]
    assert np.all(np.isfinite(got[:, fin])) and np.all(got[:, fin] >= 0.0)
    bound = 8.0 * ref_err * max(1.0, S / 1000.0)
    _hold(f"S={S} against the restatement", got, t.ref(), bound)
    if S <= 1000:
        truth = np.array([[ps.distance_both(t.x[:, p], w, ps.distance_mp) for w in (t.w_lo, t.w_hi)] for p in MP_COLS])
        _hold(f"S={S} against the 200-bit truth", got[:, MP_COLS], truth, 8.0 * ref_err)


@pytest.mark.parametrize("S", S_LIST)
def test_a_row_is_bitwise_its_own(S, synth, monkeypatch):
    t = synth(S)
    monkeypatch.delenv("NUTS_PSENS_BLOCK", raising=False)
    base = _call(t.x, t.w_lo, t.w_hi)
    for P in (1, 33, 70):
        for block in (1, 32, 1024):
            monkeypatch.setenv("NUTS_PSENS_BLOCK", str(block))
            got = _call(np.ascontiguousarray(t.x[:, :P]), t.w_lo, t.w_hi)
            assert np.array_equal(got, base[:, :P], equal_nan=True), (S, P, block)
    monkeypatch.delenv("NUTS_PSENS_BLOCK", raising=False)
    alone = _call(np.ascontiguousarray(t.x[:, 40:41]), t.w_lo, t.w_hi)          # a row alone is the row among its neighbours
    assert np.array_equal(alone[:, 0], base[:, 40])


@pytest.mark.parametrize("S", [257, 1000, 8192])
def test_tied_draws_do_not_see_the_order_of_the_trace(S, synth):
    t = synth(S)
    rng = np.random.default_rng(S)
    x = (rng.integers(0, 10 ** 6, size=(S, 9)) % 7).astype("float64")
    x[:, 8] = t.x[:, 0]                                                         # one column without ties
    base = _call(x, t.w_lo, t.w_hi)
    assert np.all(np.isfinite(base))
    for k in range(2):
        p = np.random.default_rng(k).permutation(S)
        got = _call(np.ascontiguousarray(x[p]), np.ascontiguousarray(t.w_lo[p]), np.ascontiguousarray(t.w_hi[p]))
        assert np.array_equal(got, base), (S, k)


@pytest.mark.parametrize("S", [2, 257, 1000])
def test_one_hot_weights_stay_finite(S, synth, ref_err):
    t = synth(S)
    hot, other = _one_hot(t)
    got = _call(np.ascontiguousarray(t.x[:, :5]), hot, other)
    assert np.all(np.isfinite(got)) and np.all(got[:2] > 0.0) and np.all(got[:2] <= 1.0 + 1e-12)
    ref = np.array([[ps.distance_both(t.x[:, p], w) for w in (hot, other)] for p in range(5)])
    _hold(f"S={S} one-hot weights", got, ref, 8.0 * ref_err)


def test_what_is_refused(synth):
    t = synth(3)
    for S in (1, 8193):
        with pytest.raises(ValueError, match="at least 2 draws" if S == 1 else "8192.*out of scope"):
            sensitivity.psens_from_weights(np.zeros((S, 2)), np.full(S, 1.0 / S), np.full(S, 1.0 / S), device=0)
        with pytest.raises(ValueError, match="at least 2 draws" if S == 1 else "8192"):
            sensitivity.psens_weights(np.zeros(S), 1.01, device=0)
    with pytest.raises(ValueError, match="delta"):
        sensitivity.psens_from_weights(t.x, t.w_lo, t.w_hi, delta=0.0, device=0)
    with pytest.raises(ValueError, match="3 draws, but 2"):
        sensitivity.psens_from_weights(t.x, t.w_lo[:2], t.w_hi, device=0)


# ---- nuts_psens_weights ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("S", [2, 16, 25, 100, 8192])
def test_weights_against_psis_reference(S, ties):
    rng = np.random.default_rng(50 + S)
    lc = -3.0 * rng.standard_normal(S) ** 2 - 40.0
    if ties:
        lc = np.round(lc)
        assert np.unique(lc).size < S or S == 2
    for alpha in ps.alphas():
        w, khat = sensitivity.psens_weights(lc, alpha, device=0)
        rw, rk = ps.weights(lc, alpha)
        dw = float(np.max(np.abs(w - rw) / rw))
        print("S", S, "ties", ties, "alpha", alpha, "khat", khat, "ref", rk, "max rel |w - ref|", dw, "|sum w - 1|", abs(w.sum() - 1.0))
        MEASURED[f"weights S={S} ties={ties} alpha={alpha:.6f}"] = {"khat_abs": 0.0 if khat == rk else abs(khat - rk), "w_rel": dw}
        if pr.tail_len(S) <= 4:
            raw = np.exp((alpha - 1.0) * lc - np.max((alpha - 1.0) * lc))
            assert khat == math.inf == rk
            np.testing.assert_allclose(w, raw / raw.sum(), rtol=1e-9, atol=1e-9 / S)
        elif math.isinf(rk):                 # (ties left fewer than 5 values above the cutoff)
            assert khat == rk
        else:
            np.testing.assert_allclose(khat, rk, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(w, rw, rtol=1e-9, atol=1e-9 / S)
        assert abs(math.fsum(w) - 1.0) <= S * EPS
    assert pr.tail_len(16) == 4 and pr.tail_len(25) == 5


def test_a_non_finite_log_density_poisons_the_weights():
    lc = -np.arange(40.0)
    for bad in (-np.inf, np.inf, np.nan):
        v = lc.copy()
        v[17] = bad
        w, khat = sensitivity.psens_weights(v, 1.01, device=0)
        assert np.all(np.isnan(w)) and math.isnan(khat)
    out = sensitivity.psens_from_arrays(np.random.default_rng(0).standard_normal((40, 3)), v)
    assert all(np.all(np.isnan(out[c])) for c in sensitivity.COLUMNS)


# ---- nuts_model_logdens_sum -----------------------------------------------------------------------------------------------------------------
def mixture_200():
    rng = np.random.default_rng(11)
    y = np.linspace(-2.0, 2.0, 3)[rng.integers(0, 3, size=200)] + 0.7 * rng.normal(size=200)
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 10.0, shape=3)
    sigma = m.HalfNormal("sigma", 2.0, shape=3)
    m.NormalMixture("y", ("softmax", m.Normal("logits", 0.0, 1.0, shape=3)), mu, sigma, y)
    return m.build()


def _node(spec, name):
    return next((nd[1], nd[2]) for nd in ms.observed_nodes(spec) if nd[0] == name)


NODES = {
    "factor_1": (lambda: factor_model(1), "y_studentt"),
    "factor_255": (lambda: factor_model(255), "y_studentt"),
    "factor_257": (lambda: factor_model(257), "y_poisson"),
    "factor_3000": (lambda: factor_model(3000), "y_normal"),
    "rows_32x40": (lambda: rows_model([40] * 32, 3, True)[0], "y"),
    "glm_300x5": (lambda: glm_model("normal", 5, 300, True, "var", False), "y"),
    "mixture_200": (mixture_200, "y"),
}


@pytest.mark.parametrize("label", list(NODES))
def test_totals_are_the_row_sums_and_bitwise_their_own(label, monkeypatch):
    for v in SCHED_VARS:
        monkeypatch.delenv(v, raising=False)
    build, name = NODES[label]
    spec = build()
    node = _node(spec, name)
    q = np.random.default_rng(3).normal(size=(13, spec.n)) * 0.4
    f = _vg(spec)
    try:
        ll = f.log_likelihood(name, q, node=node)
        tot = f.logdens_sum(q, node)
        N = ll.shape[1]
        bound = N * EPS * np.abs(ll).sum(axis=1)
        err = np.abs(tot - np.array([math.fsum(r) for r in ll]))
        print(label, "N", N, "max |total - fsum(row)|", err.max(), "bound", bound.min())
        assert np.all(np.isfinite(tot)) and np.all(err <= bound)
        parts = np.concatenate([f.logdens_sum(q[:1], node), f.logdens_sum(q[1:8], node), f.logdens_sum(q[8:], node)])
        assert np.array_equal(parts, tot), "a draw's total depends on how the draws were split"
        assert f.logdens_sum(q[6:7], node)[0] == tot[6], "a draw's total depends on its company"
    finally:
        f.close()
    monkeypatch.setenv("NUTS_LL_B", "1")
    f = _vg(spec)
    try:
        assert np.array_equal(f.logdens_sum(q, node), tot), "NUTS_LL_B=1 against 8"
    finally:
        f.close()


def test_a_failed_parameter_check_gives_minus_infinity():
    rng = np.random.default_rng(5)
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0)
    s = m.HalfNormal("s", 1.0, transform=None)       # untransformed: a draw may be negative
    m.Normal("y", mu, s, observed=rng.normal(size=7))
    spec = m.build()
    q = np.column_stack([rng.normal(size=11) * 0.5, 0.5 + rng.random(11)])
    q[4, 1] = -0.3
    f = _vg(spec)
    try:
        tot = f.logdens_sum(q, _node(spec, "y"))
        assert tot[4] == -np.inf and np.all(np.isfinite(np.delete(tot, 4)))
        np.testing.assert_allclose(np.delete(tot, 4), np.delete(f.log_likelihood("y", q).sum(axis=1), 4), rtol=1e-13)
    finally:
        f.close()


@pytest.mark.parametrize("N", [1, 257, 3000, 70001])
def test_dyadic_terms_sum_exactly(N):
    """y_i ~ Laplace(mu, 1/2) at integer y and mu a multiple of 1/4: every term -log(1) - 2 |y_i - mu| is a multiple of 1/2"""
    rng = np.random.default_rng(N)
    y = rng.integers(-50, 50, size=N).astype("float64")
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 10.0)
    m.Laplace("y", mu, 0.5, observed=y)
    spec = m.build()
    q = (rng.integers(-40, 40, size=(9, 1)) / 4.0).astype("float64")
    f = _vg(spec)
    try:
        tot = f.logdens_sum(q, _node(spec, "y"))
    finally:
        f.close()
    want = np.array([-(2.0 * np.abs(y - v)).sum() for v in q[:, 0]])
    assert np.array_equal(tot, want), (tot, want)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def schools():
    from pymc_amd.sampling import sample

    spec = models.eight_schools()
    res = sample(draws=200, tune=200, chains=2, model=spec, random_seed=11, device=0, psens=True)
    yield spec, res
    res["step"].close()


def _schools_host(spec, q):
    """the constrained draws and the host's log-prior (no Jacobian) and log-likelihood"""
    post = sensitivity.constrained_from_positions(spec, q)
    eta, mu, tau = post["eta"], post["mu"], post["tau"]
    lp = stats.norm.logpdf(eta).sum(axis=2) + stats.norm.logpdf(mu, 0.0, 1e6) + stats.halfcauchy.logpdf(tau, scale=25.0)
    y = np.array([28, 8, -3, 7, -1, 1, 18, 12], dtype="float64")
    sd = np.array([15, 10, 16, 11, 9, 11, 10, 18], dtype="float64")
    ll = stats.norm.logpdf(y, mu[..., None] + tau[..., None] * eta, sd).sum(axis=2)
    x = np.concatenate([eta, mu[..., None], tau[..., None]], axis=2).reshape(-1, 10)
    return x, lp, ll


def test_log_prior_holds_no_jacobian(schools):
    spec, res = schools
    q = res["draws"]
    x, lp, ll = _schools_host(spec, q)
    got = sensitivity.log_prior(spec, q, device=0)
    print("log-prior: max |device - SciPy|", np.abs(got - lp).max(), "a Jacobian would add log tau, of size", np.abs(q[..., 9]).mean())
    np.testing.assert_allclose(got, lp, rtol=1e-10, atol=1e-10)           # ten closed-form terms in float64: the project's bar for a log-density
    np.testing.assert_allclose(sensitivity.log_likelihood(spec, q, device=0), ll, rtol=1e-10, atol=1e-10)
    pw = sensitivity.compute_log_prior(spec, q, device=0)
    assert list(pw) == ["eta", "mu", "tau"] and pw["eta"].shape == (2, 200, 8) and pw["tau"].shape == (2, 200, 1)
    np.testing.assert_allclose(sum(a.sum(axis=2) for a in pw.values()), got, rtol=1e-13)
    np.testing.assert_allclose(pw["tau"][..., 0], stats.halfcauchy.logpdf(np.exp(q[..., 9]), scale=25.0), rtol=1e-10, atol=1e-10)


def test_the_table_is_the_reference_fed_the_host_arrays(schools):
    spec, res = schools
    q = res["draws"]
    x, lp, ll = _schools_host(spec, q)
    table = sensitivity.psens_table(spec, q, device=0)
    assert table["names"] == [f"eta[{i}]" for i in range(8)] + ["mu", "tau"] and table["refused"] == {}
    S = x.shape[0]
    for comp, lc in (("prior", lp), ("likelihood", ll)):
        got = sensitivity.psens(spec, q, component=comp, device=0)
        ref = ps.psens_arrays(x, lc.ravel())
        assert got["names"] == table["names"] and np.array_equal(got["sensitivity"], table[comp])
        assert (got["khat_lo"], got["khat_hi"]) == table[comp + "_khat"]
        for c in ("cjs_lo", "cjs_hi"):
            err = np.abs(got[c] ** 2 - ref[c] ** 2)
            print(comp, c, "max |D - ref|", err.max(), "D", ref[c] ** 2)
            MEASURED[f"eight schools {comp} {c}"] = {"worst_abs_error_in_D": float(err.max()), "worst_error_over_bound": float(np.max(err / (1e-8 * ref[c] ** 2 + S * EPS)))}
            # the weights are held to 1e-9 and D is at most quadratic in their tilt; S eps for the rounding of the sums
            assert np.all(err <= 1e-8 * ref[c] ** 2 + S * EPS), (comp, c)
        # khat: a fit to the 60 largest of 0.01 x lc, themselves held to 1e-10: three digits are lost at most
        np.testing.assert_allclose([got["khat_lo"], got["khat_hi"]], [ref["khat_lo"], ref["khat_hi"]], rtol=1e-6, atol=1e-6)
    assert table["diagnosis"] == ps.diagnose(table["prior"], table["likelihood"])
    ref_diag = ps.diagnose(ps.psens_arrays(x, lp.ravel())["sensitivity"], ps.psens_arrays(x, ll.ravel())["sensitivity"])
    assert table["diagnosis"] == ref_diag


def test_sample_carries_the_same_table(schools):
    spec, res = schools
    table = sensitivity.psens_table(spec, res["draws"], device=0)
    assert res["psens"]["names"] == table["names"] and res["psens"]["diagnosis"] == table["diagnosis"]
    for k in ("prior", "likelihood"):
        assert np.array_equal(res["psens"][k], table[k]) and res["psens"][k + "_khat"] == table[k + "_khat"]


@pytest.mark.parametrize("m0, s0, want", [(10.0, 0.05, "prior-data conflict"), (0.0, 100.0, "-")])
def test_a_prior_that_fights_the_data_is_diagnosed(m0, s0, want):
    """y ~ Normal(mu, 1), 20 observations centred at 0 (tests/test_psens_host.py holds the reference with exact conjugate draws to
    the same sides of 0.05, with room to spare)"""
    from pymc_amd.sampling import sample

    y = np.random.default_rng(1).standard_normal(20)
    y -= y.mean()
    m = ModelBuilder()
    mu = m.Normal("mu", m0, s0)
    m.Normal("y", mu, 1.0, observed=y)
    spec = m.build()
    res = sample(draws=200, tune=200, chains=2, model=spec, random_seed=3, device=0, psens=True)
    try:
        t = res["psens"]
        print("mu ~ Normal(%g, %g): prior" % (m0, s0), t["prior"], "likelihood", t["likelihood"], t["diagnosis"])
        assert t["names"] == ["mu"] and t["diagnosis"] == [want]
        if want == "-":
            assert t["prior"][0] < 0.0125
        else:
            assert t["prior"][0] > 0.2 and t["likelihood"][0] > 0.2
    finally:
        res["step"].close()


def test_a_refused_component_leaves_the_other():
    """a Potential that reads a variable: the prior component is refused by name, the likelihood's column stays"""
    y = np.linspace(-1.0, 1.0, 12)
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0, shape=2)
    m.Potential("push", -(a * a))
    m.Normal("y", a[np.arange(12) % 2], 1.0, observed=y)
    spec = m.build()
    q = np.random.default_rng(2).normal(size=(1, 60, spec.n)) * 0.3
    t = sensitivity.psens_table(spec, q, device=0)
    assert list(t["refused"]) == ["prior"] and "Potentials out of compute_log_prior" in t["refused"]["prior"]
    assert np.all(np.isnan(t["prior"])) and np.all(np.isfinite(t["likelihood"])) and t["diagnosis"] == ["-", "-"]
    with pytest.raises(ValueError, match="log-prior refused"):
        sensitivity.psens(spec, q, component="prior", device=0)
