"""The linear-predictor node (dense node 5, pymc_amd/csrc/lin_kernel.h) at its shape edges, on the device, against EXACT ARITHMETIC
(tests/lin_edges.py; the host side is tests/test_lin_edges.py, which also holds the CPU oracle to the same references).

Everything goes through `DeviceValueGradFunction`, at three positions per model.

  * The integer family (`lin_edges.exact_model`): the gradient must be BITWISE the exact one -- `np.array_equal` against exact
    arithmetic, not against the oracle and not within a tolerance -- and the log-density within its counted bound (only the priors'
    terms and the additions behind them round).  The shapes (`lin_edges.EXACT_CASES`) are every instantiation `KT` full and partly
    filled, both sides of a forward workgroup (256 rows) and of a backward chunk (2048 rows), the forward grid's second trip
    (N = 4096 * 256 + 257), P = 512, K P = 4096 both ways, two to four readers of a column (`lin_adj`), derived coefficients, one
    vector against two matrices (`LinTarget.n_src` = 2) and the one-row kernels around their trip of 8 x 1024 elements.
  * The same bits under every route of the adjoint sweep and of the small-model switch.  The single-workgroup kernel never takes a
    model with a linear predictor (`single_workgroup_ok` is 0 for every case here), so NUTS_SMALL_KERNEL must change nothing.
  * Element by element: the likelihood marked `observed`, `loglik.compute_log_likelihood` row by row against -0.5 (y_i - eta_i)^2,
    bitwise; a failure names the first wrong row and its workgroup and chunk.
  * The real-valued family within the bound COUNTED from the kernels (`lin_edges.rounding_count`); with PYMC_AMD_LIN_EDGES_JSON set
    to a path the run writes the largest error per case as a fraction of its bound there (profiles/lin_edges.json).
  * NUTS over a two-reader model carries the oracle sampler's integers.
  * A column, and a whole predictor, that no factor reads (only a Deterministic, which the host evaluates): `k_lin_bwd` does not
    touch the adjoint table for it, the launch leaves a predictor without readers out.  Every such case here has at least as many
    swept adjoint elements as the unread predictor has rows, so that the kernel before the fix would have read inside its buffer
    as well (DESIGN.md 4.12 has the argument for the other shapes).
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lin_edges as le  # noqa: E402

from oracle import ref_models, ref_sampler  # noqa: E402
from pymc_amd import model_spec as ms  # noqa: E402

pytestmark = pytest.mark.gpu


def _device(spec):
    from pymc_amd.value_grad import DeviceValueGradFunction

    assert spec.lins and ms.engine_refusal(spec) is None
    f = DeviceValueGradFunction(spec, device=0)
    # the lin kernels ran: the model has predictors, the engine accepted it, and the single-workgroup kernel (which has no
    # linear-predictor phase) is not an option for it -- `launch_vector` is the only way to a gradient
    assert f.model_scalar("single_workgroup_ok") == 0.0
    return f


def _hold_exact(model, refs, f, route=""):
    C = le.logp_rounding_count(model)
    for i, (q, ex) in enumerate(refs):
        lp, g = f._pytensor_function(q)
        want = ex.grad_floats()
        print(f"{model.label}{route} position {i}: |logp - exact| = {abs(lp - ex.logp_float()):.3e}, bound {le.bound(C, ex.S_logp):.3e}; "
              f"gradient elements wrong: {int(np.sum(g != want))} of {len(want)}")
        assert np.array_equal(g, want), route + le.gradient_message(model, g, want)
        assert abs(lp - ex.logp_float()) <= le.bound(C, ex.S_logp) + le.U * abs(ex.logp_float()), (model.label, route, lp, ex.logp_float())
        lp2, g2 = f._pytensor_function(q)      # nothing is atomic: the same bits every time
        assert lp2 == lp and np.array_equal(g2, g)


@pytest.mark.parametrize("name", sorted(le.EXACT_CASES))
def test_gradient_is_exact_arithmetic_bit_for_bit(name):
    model = le.exact_case(name)
    f = _device(model.spec)
    try:
        _hold_exact(model, le.reference("exact", name), f)
    finally:
        f.close()


ROUTES = [("NUTS_GSWEEP_FAST", "0"), ("NUTS_GSWEEP_LDS", "0"), ("NUTS_SMALL_KERNEL", "0"), ("NUTS_SMALL_KERNEL", "1")]


@pytest.mark.parametrize("var,value", ROUTES, ids=[f"{k}={v}" for k, v in ROUTES])
def test_every_route_gives_the_bits_of_exact_arithmetic(var, value, monkeypatch):
    monkeypatch.setenv(var, value)
    for name in le.ROUTE_CASES:
        model = le.exact_case(name)
        f = _device(model.spec)
        try:
            _hold_exact(model, le.reference("exact", name), f, route=f" [{var}={value}] ")
        finally:
            f.close()


@pytest.mark.parametrize("name", le.LOGLIK_CASES)
def test_pointwise_log_likelihood_is_exact_row_by_row(name):
    from pymc_amd import loglik

    model = le.exact_model(**le.EXACT_CASES[name])      # (a model of its own: the shared one is not marked)
    model.spec.factors[model.factor_index("y")].observed = True
    refs = le.reference("exact", name)
    q = np.stack([q for q, _ in refs])
    f = _device(model.spec)
    try:
        got = loglik.compute_log_likelihood(model.spec, q[None], func=f)["y"][0]
    finally:
        f.close()
    N = model.Xs[0].shape[0]
    assert got.shape == (len(refs), N)
    for s, (_, ex) in enumerate(refs):
        want = ex.loglik.floats()
        assert want.shape == (N,) and np.any(want != 0.0)
        i = le.first_wrong(got[s], want)
        assert i is None, f"{model.label}, position {s}: {le.where(i)}: device {got[s][i]!r}, exact {want[i]!r}; {int(np.sum(got[s] != want))} of {N} rows wrong"


_profile = {}


def _write_profile():
    path = os.environ.get("PYMC_AMD_LIN_EDGES_JSON")
    if path:
        with open(path, "w") as fh:
            json.dump(_profile, fh, indent=1, sort_keys=True)
            fh.write("\n")


@pytest.mark.parametrize("name", sorted(le.REAL_CASES))
def test_real_valued_models_stay_inside_the_counted_bound(name):
    model = le.real_case(name)
    C, Cl = le.rounding_count(model), le.logp_rounding_count(model)
    f = _device(model.spec)
    ent = {"C_grad": C, "C_logp": Cl, "positions": []}
    try:
        failures = []
        for i, (q, ex) in enumerate(le.reference("real", name)):
            lp, g = f._pytensor_function(q)
            lp_o, g_o = ref_models.evaluate(model.spec, q)
            want, wlp = ex.grad_floats(), ex.logp_float()
            lim = le.bound(C, ex.S_grad) + le.U * np.abs(want)               # (+ the reference's own conversion to float64)
            llim = le.bound(Cl, ex.S_logp) + le.U * abs(wlp)
            frac, frac_o = np.abs(g - want) / lim, np.abs(g_o - want) / lim
            w = int(np.argmax(frac))
            ent["positions"].append({
                "grad_worst_fraction_of_bound": {"device": float(frac[w]), "oracle": float(np.max(frac_o)), "element": w},
                "grad_at_worst": {"device": float(g[w]), "oracle": float(g_o[w]), "exact": float(want[w]), "bound": float(lim[w])},
                "logp_fraction_of_bound": {"device": abs(lp - wlp) / llim, "oracle": abs(lp_o - wlp) / llim},
                "logp": {"device": float(lp), "oracle": float(lp_o), "exact": wlp, "bound": llim}})
            print(f"{name} position {i}: gradient at {float(frac[w]):.4f} of its bound (element {w}; oracle {float(np.max(frac_o)):.4f}), "
                  f"logp at {abs(lp - wlp) / llim:.4f} of its bound (oracle {abs(lp_o - wlp) / llim:.4f})")
            if not np.all(frac <= 1.0):
                failures.append((i, "gradient", w, float(frac[w])))
            if not abs(lp - wlp) <= llim:
                failures.append((i, "logp", lp, wlp, llim))
        _profile[name] = ent
        _write_profile()
        assert not failures, (name, failures)
    finally:
        f.close()


def test_nuts_carries_the_oracle_samplers_integers():
    from pymc_amd.sampling import sample

    spec = le.real_model(**le.NUTS_CASE).spec
    assert ms.engine_refusal(spec) is None
    res = sample(draws=8, tune=16, chains=1, model=spec, init="adapt_diag", random_seed=21, device=0)
    _, ref_stats = ref_sampler.sample_reference(ref_models.SpecLogpGrad(spec), [np.zeros(spec.n)], draws=8, tune=16, random_seed=21, init="adapt_diag")
    dev = res["warmup_stats"][0] + res["stats"][0]
    res["step"].close()
    same = sum(all(int(a[k]) == int(b[k]) for k in ("depth", "tree_size", "index_in_trajectory", "diverging")) for a, b in zip(dev, ref_stats[0]))
    assert same == len(dev), (same, len(dev))


def test_the_engine_refuses_a_fifth_reader_in_the_words_the_host_uses():
    from pymc_amd import _lib
    from pymc_amd.value_grad import DeviceValueGradFunction

    spec = le.exact_model(N=8, P=2, readers=5).spec
    why = ms.engine_refusal(spec)
    assert why and "LIN_MAXUSE" in why
    with pytest.raises(_lib.EngineError) as err:
        DeviceValueGradFunction(spec, device=0)
    assert why in str(err.value)
    f = _device(le.exact_model(N=8, P=2, readers=4).spec)
    f.close()


# ---- columns and predictors that no factor reads ----------------------------------------------------------------------------------------
def test_an_unread_column_gets_the_priors_gradient_and_its_neighbours_stay_exact():
    """K = 3, column 2 read by nobody: 2 x 300 swept adjoint elements, 300 rows."""
    model = le.exact_case("unread-column")
    f = _device(model.spec)
    try:
        _hold_exact(model, le.reference("exact", "unread-column"), f)
        for q, _ in le.reference("exact", "unread-column"):
            _, g = f._pytensor_function(q)
            assert np.array_equal(g.reshape(model.P, model.K)[:, 2], -q.reshape(model.P, model.K)[:, 2])
    finally:
        f.close()


@pytest.mark.parametrize("n_unread", [4, 3])
def test_a_predictor_only_a_deterministic_reads(n_unread):
    """The model of tests/test_lin_node.py's Deterministic test (4 swept adjoint elements; the unread predictor has 4 rows, or 3)."""
    spec, X, _ = le.deterministic_model(n_unread)
    f = _device(spec)
    try:
        for q in (np.zeros(3), np.array([0.5, -1.0, 2.0]), np.array([-0.125, 1.75, 0.25])):
            lp, g = f._pytensor_function(q)
            lp0, _ = ref_models.evaluate(spec, q)
            assert np.array_equal(g, X.T @ (0.0 - X @ q) - q)                # small dyadic numbers: exact in float64
            assert abs(lp - lp0) <= 64 * le.U * abs(lp0)      # (every term is negative, so |lp0| is their absolute sum; far fewer than 64 roundings, the oracle's included)
    finally:
        f.close()
