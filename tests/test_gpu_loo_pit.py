"""LOO predictive checks on the device (csrc/psis.h psis_fit / psis_weight, csrc/loo_pit_kernel.h, `nuts_loo_pit_*`,
`predictive.loo_pit`).

Reference: the NumPy restatement (tests/loo_pit_reference.py: whole vectors, the tie-mean rule) applied to the device's OWN [S][N]
matrices from `compute_log_likelihood` and `sample_posterior_predictive` -- both are held to their own references elsewhere, and a
draw's values do not depend on its batch (tested there, bit for bit), so the second pass sees exactly the values the reference gets
and the comparison isolates the new arithmetic: the weight of a draw from the streamed state, and the weighted folds.

Conditions, asserted on the reference before anything is compared: every observation's values span less than 600 nats (beyond
that the linear-scale normaliser of the fit underflows), every elpd_loo_i is finite, and no observation is left out.

Bars: p_lt, p_eq, loo_mean, loo_sd and ess at rtol = atol = 1e-9 (the project's bar for these accumulators), sum_w within 1e-12
of 1, pareto_k and loo_i equal to `loglik.loo`'s.

The models, scales and seeds are those of tests/test_gpu_psis.py; each model's trace of 203 draws is evaluated once, S = 20, 21,
37, 203 are its prefixes (S = 20: no tail is fitted; 21: the smallest fit; none is a multiple of the batch of 8).

With PYMC_AMD_LOO_PIT_JSON set to a path, the run writes the measured maxima there (profiles/loo_pit.json).
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loo_pit_reference as lr  # noqa: E402
from test_gpu_loglik import factor_model, glm_model, mix_model, rows_model  # noqa: E402

from pymc_amd import loglik, models, predictive  # noqa: E402
from pymc_amd import model_spec as ms  # noqa: E402
from pymc_amd.model_spec import ModelBuilder  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-9, atol=1e-9)
S_ALL = 203
S_LIST = [20, 21, 37, 203]
SEED = 0x5EED0123456789AB
COMPARED = ("p_lt", "p_eq", "loo_mean", "loo_sd", "ess")
MEASURED = {}


def _rows():
    spec, _, y, _ = rows_model([1, 70, 129, 33], 3, False)
    return spec, y.astype("float64")


def _observed(spec, name):
    """the observed vector of `name`, in the caller's order"""
    _, kind, index, _ = next(nd for nd in ms.observed_nodes(spec) if nd[0] == name)
    if kind == ms.LL_FACTOR:
        return np.array(spec.data[spec.factors[index].args[0].a.ref], dtype="float64")
    if kind == ms.LL_GLM:
        return np.array(spec.glm_rows.y, dtype="float64")
    assert kind == ms.LL_MIXTURE
    return np.array(spec.mixture_rows.y, dtype="float64")


# label -> (spec builder giving (spec, y or None), observed variable, scale of the draws, seed)
MODELS = {
    "factor_1": (lambda: (factor_model(1), None), "y_studentt", 0.5, 1),
    "factor_257": (lambda: (factor_model(257), None), "y_studentt", 0.5, 1),
    "glm_1000x3": (lambda: (glm_model("bernoulli", 3, 1000, True, None, False), None), "y", 1.0, 2),
    "rows_unequal_groups": (_rows, "y", 0.75, 3),
    "mixture": (lambda: (mix_model("dirichlet"), None), "y", 0.5, 4),
}


def _vg(spec):
    from pymc_amd.value_grad import DeviceValueGradFunction

    return DeviceValueGradFunction(spec, device=0)


class Trace:
    """One model, its 203 draws and the device's own values and replicates of them (caller's order), evaluated once and left
    unchanged."""

    def __init__(self, label):
        build, self.name, scale, seed = MODELS[label]
        self.label = label
        self.spec, y = build()
        self.y = _observed(self.spec, self.name) if y is None else y
        self.q = np.random.default_rng(seed).normal(size=(S_ALL, self.spec.n)) * scale
        self.f = _vg(self.spec)
        self.ll = loglik.compute_log_likelihood(self.spec, self.q[None], var_names=[self.name], func=self.f)[self.name][0]
        self.yrep = predictive.sample_posterior_predictive(self.spec, self.q[None], var_names=[self.name], random_seed=SEED, func=self.f)[self.name][0]
        assert self.ll.shape == self.yrep.shape == (S_ALL, self.y.size)
        for a in (self.ll, self.yrep, self.y):
            a.setflags(write=False)
        self._ref = {}

    def ref(self, S):
        if S not in self._ref:
            self._ref[S] = _reference(self.ll[:S], self.yrep[:S], self.y)
        return self._ref[S]


def _reference(ll, yrep, y):
    """the restatement, after the stated conditions"""
    span = ll.max(axis=0) - ll.min(axis=0)
    assert np.all(span < 600.0), float(span.max())
    ref = lr.loo_pit_matrix(ll, yrep, y)
    assert all(np.all(np.isfinite(ref[k])) for k in lr.COLUMNS), "an observation would be left out"
    return ref


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
    path = os.environ.get("PYMC_AMD_LOO_PIT_JSON")
    if path and MEASURED:
        with open(path, "w") as fh:
            json.dump(MEASURED, fh, indent=1, sort_keys=True)


def _compare(label, got, ref, S):
    n = ref["p_lt"].size
    rec = {"left_out": 0}
    for k in COMPARED:
        assert got[k].shape == (n,) and np.all(np.isfinite(got[k])), (label, k)
        rec[k] = float(np.max(np.abs(got[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))))
    rec["sum_w"] = float(np.max(np.abs(got["sum_w"] - 1.0)))
    print(label, "S", S, "largest differences", rec)
    MEASURED[f"{label}/S={S}"] = rec
    for k in COMPARED:
        np.testing.assert_allclose(got[k], ref[k], err_msg=f"{label} S={S} {k}", **TOL)
    assert np.all(np.abs(got["sum_w"] - 1.0) <= 1e-12), (label, rec["sum_w"])
    assert np.array_equal(got["loo_pit"], got["p_lt"] + got["p_eq"]) and np.array_equal(got["loo_pit_mid"], got["p_lt"] + 0.5 * got["p_eq"])
    assert np.all((got["loo_pit"] >= 0.0) & (got["loo_pit"] <= 1.0 + 1e-12))


@pytest.mark.parametrize("S", S_LIST)
@pytest.mark.parametrize("label", list(MODELS))
def test_loo_pit_against_the_restatement_on_the_devices_own_values(label, S, traces):
    t = traces(label)
    ref = t.ref(S)
    got = predictive.loo_pit(t.spec, t.q[None, :S], var_name=t.name, random_seed=SEED, func=t.f)
    _compare(label, got, ref, S)
    first = loglik.loo(t.spec, t.q[None, :S], var_name=t.name, pointwise=True, func=t.f)
    assert np.all(np.isfinite(first["loo_i"]))
    for k in first:
        assert np.array_equal(got[k], first[k]), k
    if S == 20:
        assert np.all(got["pareto_k"] == np.inf)             # nothing is smoothed: the weights are the raw ratios
    if label in ("glm_1000x3", "rows_unequal_groups"):
        assert np.all(np.isin(t.y, (0.0, 1.0))) and np.any(got["p_eq"] > 0.0)      # Bernoulli: y_rep == y has weight
    else:
        assert np.all(got["p_eq"] == 0.0)                    # continuous data


def _second_pass(t, first, pieces, q=None, seed=SEED):
    q = t.q if q is None else q
    acc = t.f.loo_pit_accumulator(first, seed=seed)
    try:
        s0 = 0
        for k in pieces:
            acc.update(q[s0:s0 + k], draw0=s0)
            s0 += k
        return acc.read()
    finally:
        acc.close()


def test_the_state_does_not_depend_on_how_the_draws_were_split(traces):
    t = traces("glm_1000x3")
    first = t.f.psis_accumulator(t.name, S_ALL)
    try:
        first.update(t.q)
        reads = [_second_pass(t, first, split) for split in ([S_ALL], [5, 8, 190], [1] * S_ALL)]
    finally:
        first.close()
    assert reads[0][6] == S_ALL
    for other in reads[1:]:
        assert other[6] == S_ALL
        for a, b in zip(reads[0][:6], other[:6]):
            assert np.array_equal(a, b), "the state depends on how the draws were split"
    # and it is the restatement's (evaluation order = the caller's for a GLM node)
    ref = t.ref(S_ALL)
    np.testing.assert_allclose(reads[0][0], ref["p_lt"], **TOL)
    np.testing.assert_allclose(reads[0][3], ref["loo_sd"] ** 2, **TOL)


@pytest.mark.parametrize("label", ["glm_1000x3", "factor_257"])
def test_batch_of_one_against_eight(label, traces, monkeypatch):
    t = traces(label)
    want = predictive.loo_pit(t.spec, t.q[None, :37], var_name=t.name, random_seed=SEED, func=t.f)
    monkeypatch.setenv("NUTS_LL_B", "1")
    f = _vg(t.spec)
    try:
        got = predictive.loo_pit(t.spec, t.q[None, :37], var_name=t.name, random_seed=SEED, func=f)
    finally:
        f.close()
    for k in want:
        assert np.array_equal(got[k], want[k]), ("NUTS_LL_B=1 against 8", k)


def test_two_chains_pooled_are_the_concatenated_trace(traces):
    t = traces("rows_unequal_groups")
    one = predictive.loo_pit(t.spec, t.q[None, :202], var_name=t.name, random_seed=SEED, func=t.f)
    two = predictive.loo_pit(t.spec, t.q[:202].reshape(2, 101, -1), var_name=t.name, random_seed=SEED, chain_ids=(0, 1), func=t.f)
    assert one["n_samples"] == two["n_samples"] == 202
    for k in one:
        assert np.array_equal(one[k], two[k]), k
    # results are in the CALLER's row order: the rows were passed unsorted
    assert t.spec.rows_order is not None
    _compare("rows pooled", two, _reference(t.ll[:202], t.yrep[:202], t.y), 202)
    # other chain numbers are other replicates
    far = predictive.loo_pit(t.spec, t.q[:202].reshape(2, 101, -1), var_name=t.name, random_seed=SEED, chain_ids=(0, 5), func=t.f)
    assert np.array_equal(far["loo_i"], one["loo_i"]) and not np.array_equal(far["loo_mean"], one["loo_mean"])


def test_duplicated_draws_give_the_same_result_in_either_order(traces):
    """Every draw occurs twice: every value of the tail is tied.  Replicates are addressed by draw NUMBER, so the two orders are
    compared through the restatement on each order's own matrices, and directly where the replicate does not enter (the weights)."""
    t = traces("factor_257")
    half = 100
    q_ab = np.concatenate([t.q[:half], t.q[:half]])
    perm = np.random.default_rng(12).permutation(2 * half)
    q_perm = q_ab[perm]
    outs = []
    for label, q in (("duplicated", q_ab), ("duplicated, permuted", q_perm)):
        ll = loglik.compute_log_likelihood(t.spec, q[None], var_names=[t.name], func=t.f)[t.name][0]
        yrep = predictive.sample_posterior_predictive(t.spec, q[None], var_names=[t.name], random_seed=SEED, func=t.f)[t.name][0]
        got = predictive.loo_pit(t.spec, q[None], var_name=t.name, random_seed=SEED, func=t.f)
        _compare("factor_257 " + label, got, _reference(ll, yrep, t.y), 2 * half)
        outs.append(got)
    # the weights themselves (ess, the first pass) do not know the order
    np.testing.assert_allclose(outs[0]["ess"], outs[1]["ess"], rtol=1e-12)
    # (the sorted column is the same in either order, so is khat; the running sum of the rest adds up to 160 terms in another order)
    assert np.array_equal(outs[0]["pareto_k"], outs[1]["pareto_k"])
    np.testing.assert_allclose(outs[0]["loo_i"], outs[1]["loo_i"], rtol=1e-12, atol=1e-12)
    # with one seed per HALF the replicates of a pair are the same number in either order: then everything agrees
    first = t.f.psis_accumulator(t.name, 2 * half)
    try:
        first.update(q_ab)
        a = t.f.loo_pit_accumulator(first, seed=SEED)
        b = t.f.loo_pit_accumulator(first, seed=SEED)
        try:
            a.update(t.q[:half], draw0=0); a.update(t.q[:half], draw0=half)
            b.update(t.q[:half], draw0=half); b.update(t.q[:half], draw0=0)
            ra, rb = a.read(), b.read()
        finally:
            a.close()
            b.close()
    finally:
        first.close()
    for u, v in zip(ra[:6], rb[:6]):
        np.testing.assert_allclose(u, v, rtol=1e-12, atol=1e-12)      # (200 folds of doubles of magnitude 1 in another order)


def test_a_degenerate_fit_gives_nan_for_that_observation_only():
    """A failed parameter check (an untransformed scale below 0) kills factor `y` at that draw: ll = -inf there, elpd_loo_i = -inf, and
    every column of each of its observations is NaN; `y2`, which does not read the scale, is finite everywhere."""
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
    f = _vg(spec)
    try:
        got = predictive.loo_pit(spec, q[None], var_name="y", random_seed=SEED, func=f)
        for k in ("loo_pit", "loo_pit_mid", "p_lt", "p_eq", "loo_mean", "loo_sd", "ess", "sum_w"):
            assert got[k].shape == (7,) and np.all(np.isnan(got[k])), k
        assert np.all(got["loo_i"] == -np.inf) and np.all(got["pareto_k"] == np.inf)
        got2 = predictive.loo_pit(spec, q[None], var_name="y2", random_seed=SEED, func=f)
        ll = loglik.compute_log_likelihood(spec, q[None], var_names=["y2"], func=f)["y2"][0]
        yrep = predictive.sample_posterior_predictive(spec, q[None], var_names=["y2"], random_seed=SEED, func=f)["y2"][0]
        _compare("degenerate/y2", got2, _reference(ll, yrep, _observed(spec, "y2")), S)
    finally:
        f.close()


def test_other_draws_in_the_second_pass_are_noticed(traces):
    t = traces("factor_257")
    S = 37
    first = t.f.psis_accumulator(t.name, S)
    try:
        first.update(t.q[:S])
        elpd, khat, lppd, _ = first.read()
        cols = _second_pass(t, first, [S], q=t.q[100:100 + S])
        with pytest.raises(ValueError, match="the second pass did not see the draws of the first"):
            predictive.loo_pit_from_accumulators(*cols[:6], elpd, khat, lppd, S)
        cols = _second_pass(t, first, [S - 1])          # one draw short
        with pytest.raises(ValueError, match="the second pass did not see the draws of the first"):
            predictive.loo_pit_from_accumulators(*cols[:6], elpd, khat, lppd, S)
        acc = t.f.loo_pit_accumulator(first, seed=SEED)
        try:
            acc.update(t.q[:30])
            with pytest.raises(ValueError, match="exceed the 37"):
                acc.update(t.q[:8], draw0=30)
            with pytest.raises(ValueError, match="below 2\\^32"):
                acc.update(t.q[:2], draw0=2 ** 32 - 1)
            acc.update(t.q[30:S], draw0=30)
            predictive.loo_pit_from_accumulators(*acc.read()[:6], elpd, khat, lppd, S)       # (refused calls changed nothing)
        finally:
            acc.close()
    finally:
        first.close()
    short = t.f.psis_accumulator(t.name, S)
    try:
        short.update(t.q[:13])
        with pytest.raises(ValueError, match="13 of 37 draws"):
            t.f.loo_pit_accumulator(short, seed=SEED)
    finally:
        short.close()


def test_a_binomial_likelihood_is_refused_by_name_before_anything_runs():
    spec = factor_model(7)
    with pytest.raises(ValueError, match="y_binomial.*Binomial"):
        predictive.loo_pit(spec, np.zeros((1, 4, spec.n)), var_name="y_binomial", device=0)
    f = _vg(spec)
    try:
        p = f.psis_accumulator("y_binomial", 4)
        try:
            p.update(np.zeros((4, spec.n)))
            with pytest.raises(ValueError, match="Binomial is out of scope"):
                f.loo_pit_accumulator(p)
        finally:
            p.close()
    finally:
        f.close()
    from pymc_amd.sampling import sample

    with pytest.raises(ValueError, match="loo_pit=True refused.*Binomial"):
        sample(draws=5, tune=5, chains=1, model=spec, random_seed=1, device=0, loo_pit=True)


def test_sample_returns_the_loo_pit_group_on_request():
    from pymc_amd.sampling import sample

    spec = models.eight_schools()
    res = sample(draws=20, tune=20, chains=2, model=spec, random_seed=19, device=0, loo_pit=True)
    try:
        lp = res["loo_pit"]
        assert list(lp) == ["obs"]
        out = lp["obs"]
        for k in ("loo_pit", "loo_pit_mid", "p_lt", "p_eq", "loo_mean", "loo_sd", "ess", "pareto_k", "loo_i", "sum_w"):
            assert out[k].shape == (8,) and np.all(np.isfinite(out[k]) | (k == "pareto_k")), k
        assert np.all((out["loo_pit"] >= 0.0) & (out["loo_pit"] <= 1.0)) and out["n_samples"] == 40
        again = predictive.loo_pit(spec, res, random_seed=predictive.seed_from(19), device=0)
        for k in out:
            assert np.array_equal(again[k], out[k]), k
    finally:
        res["step"].close()
    res = sample(draws=5, tune=5, chains=1, model=spec, random_seed=19, device=0)
    assert "loo_pit" not in res
    res["step"].close()
