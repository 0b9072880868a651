"""The device's scalar ops against mpmath at the edges of their domains (csrc/scalar_math.h and the device library's lgamma, erf,
erfc, erfcx, pow, ... inside csrc/model_dev.h `prog_op_value` / `prog_op_adjoint`), element by element.

Isolation: `Potential(s * op(x))` over Flat vectors at s = 1, so grad[s_i] is op(x_i) and grad[x_i] is op'(x_i) with no sum in
between (tests/scalar_edges.py; bit-exact on the oracle, tests/test_scalar_edges.py).  Routes: element-aligned operands (kernels
B / C: carries the accuracy assertion), and the same ops through `x[idx]`, idx a fixed permutation, under the resolved-operand sweep
(k_gsweep_fast), the generic sweep (NUTS_GSWEEP_FAST = 0) and without a sweep (NUTS_GSWEEP = 0): all four share `prog_op_value` /
`prog_op_adjoint` and must agree bit for bit.  Measure and bound: every regime's error E_dev <= 16 max(1, E_O), E_O the oracle's
error on the same points (tests/scalar_edges.py).  Points where the truth or the oracle is not finite are held to the oracle's
class (finite, +inf, -inf, NaN) only, in a model of their own.

Densities: observed factors whose parameters are Flat vectors, at the arguments that take the branches of `dist_eval_body` no
other test reaches (the truncated normal's three normalisers with erfcx, the `logpow` special cases, z = 1e150 ...): the element-wise
log-density through `log_likelihood` (k_ll_factor), the partials w.r.t. the parameters through the gradient, same measure and bound.

Free variables: the gradient of a free vector with constant parameters is d/dq (logp(x(q)) + log|dx/dq|) element by element: the
densities' d0 without a transform, and the log, log-odds and interval transforms at q = +-1e-8 ... +-700 (transform_full).

With PYMC_AMD_SCALAR_EDGES_JSON set to a path, the run writes every regime's E_dev there (profiles/scalar_edges.json).
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scalar_edges as se  # noqa: E402

pytestmark = pytest.mark.gpu

ROUTES = {"aligned": (False, {}), "gathered_fast": (True, {}), "gathered_generic": (True, {"NUTS_GSWEEP_FAST": "0"}),
          "gathered_no_sweep": (True, {"NUTS_GSWEEP": "0"})}


def _evaluate(groups, gather, env):
    from pymc_amd.value_grad import DeviceValueGradFunction

    spec, q, layout = se.build_model(groups, gather=gather)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        f = DeviceValueGradFunction(spec, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        lp, grad = f._pytensor_function(q)
    finally:
        f.close()
    return float(lp), [se.read_outputs(where, grad) for where in layout]


@pytest.fixture(scope="module")
def runs():
    """{route: {model: (log-density, [(op, selection, outputs)])}}: every model once per route"""
    models = se.accuracy_groups() + [("conventions", se.convention_groups())]
    out = {}
    for route, (gather, env) in ROUTES.items():
        out[route] = {}
        for name, g in models:
            lp, outs = _evaluate(se.group_points(g), gather, env)
            out[route][name] = (lp, [(op, sel, o) for (op, sel), o in zip(g, outs)])
    return out


def _per_op(run):
    """outputs over all points of POINTS[op], gathered from the accuracy models of one route"""
    full = {}
    for name, (_, groups) in run.items():
        if name == "conventions":
            continue
        for op, sel, o in groups:
            se.scatter(op, sel, o, full.setdefault(op, {}))
    return full


@pytest.fixture(scope="module")
def device_errors(runs):
    full = _per_op(runs["aligned"])
    errs = {}
    for op in se.POINTS:
        errs.update(se.regime_errors(op, full[op]))
    _write_profile({k: {"E_dev": errs[k], "E_O": se.E_O[k], "bound": se.bound(k)} for k in sorted(errs)})
    return errs


def _write_profile(entries):
    path = os.environ.get("PYMC_AMD_SCALAR_EDGES_JSON")
    if not path:
        return
    old = {}
    if os.path.exists(path):
        with open(path) as fh:
            old = json.load(fh)
    old.update(entries)
    with open(path, "w") as fh:
        json.dump(old, fh, indent=1, sort_keys=True)


def test_every_accuracy_model_has_a_finite_log_density(runs):
    for route, run in runs.items():
        for name, (lp, _) in run.items():
            assert name == "conventions" or np.isfinite(lp), (route, name, lp)


@pytest.mark.parametrize("op", sorted(se.POINTS))
def test_every_regime_of_the_op_is_within_its_bound(device_errors, op):
    mine = {k: e for k, e in device_errors.items() if k.startswith(op + "/")}
    assert set(mine) == {k for k in se.E_O if k.startswith(op + "/")}
    for k, e in mine.items():
        print(f"{k}: E_dev = {e:.4g}, E_O = {se.E_O[k]:.4g}, bound {se.bound(k):.4g}")
    bad = {k: (e, se.bound(k)) for k, e in mine.items() if not e <= se.bound(k)}
    assert not bad, bad


@pytest.mark.parametrize("route", [r for r in ROUTES if r != "aligned"])
def test_the_routes_agree_bit_for_bit(runs, route):
    for name, (_, groups) in runs["aligned"].items():
        for (op, _, want), (_, _, got) in zip(groups, runs[route][name][1]):
            for o in want:
                assert np.array_equal(got[o] + 0.0, want[o] + 0.0, equal_nan=True), (name, op, o, got[o], want[o])


def test_the_conventions_are_the_oracles(runs):
    """same class (finite, +inf, -inf, NaN) as the oracle, output by output, and a zero derivative where the oracle's is zero"""
    _, groups = runs["aligned"]["conventions"]
    bad = []
    for op, pts, got in groups:
        want = se.oracle_outputs(op, pts)
        for o in want:
            for p, a, b in zip(pts, got[o], want[o]):
                if se.klass(a) != se.klass(b) or (b == 0.0 and a != 0.0):
                    bad.append((op, o, tuple(p), a, b))
    assert not bad, bad


@pytest.fixture(scope="module")
def density_errors():
    from pymc_amd.value_grad import DeviceValueGradFunction

    errs = {}
    for name, cases in se.density_models():
        spec, q, layout = se.build_density_model(cases)
        f = DeviceValueGradFunction(spec, device=0)
        try:
            lp, grad = f._pytensor_function(q)
            assert np.isfinite(lp), (name, lp)
            for c, where in zip(cases, layout):
                out = {"lp": f.log_likelihood(c["name"], q[None, :])[0]}
                for k, ix in enumerate(where):
                    out[f"d{k + 1}"] = grad[ix]
                errs.update(se.density_errors(c["ci"], out))
        finally:
            f.close()
    _write_profile({k: {"E_dev": errs[k], "E_O": se.E_O_DENSITY[k], "bound": se.density_bound(k)} for k in sorted(errs)})
    return errs


def test_every_density_case_is_within_its_bound(density_errors):
    assert set(density_errors) == set(se.E_O_DENSITY)
    for k, e in density_errors.items():
        print(f"{k}: E_dev = {e:.4g}, E_O = {se.E_O_DENSITY[k]:.4g}, bound {se.density_bound(k):.4g}")
    bad = {k: (e, se.density_bound(k)) for k, e in density_errors.items() if not e <= se.density_bound(k)}
    assert not bad, bad


@pytest.fixture(scope="module")
def free_runs():
    from pymc_amd.value_grad import DeviceValueGradFunction

    out = {}
    for name, sel in se.free_models():
        spec, q, where = se.build_free_model(sel)
        f = DeviceValueGradFunction(spec, device=0)
        try:
            lp, grad = f._pytensor_function(q)
        finally:
            f.close()
        out[name] = (float(lp), sel, {case: grad[ix] for case, ix in where.items()})
    return out


def test_free_variables_and_transforms_are_within_their_bounds(free_runs):
    errs = {}
    for name in ("free", "free_huge"):
        lp, sel, grads = free_runs[name]
        assert np.isfinite(lp), (name, lp)
        se.free_errors(grads, sel, errs)
    assert set(errs) == set(se.E_O_FREE)
    _write_profile({k: {"E_dev": errs[k], "E_O": se.E_O_FREE[k], "bound": se.free_bound(k)} for k in sorted(errs)})
    for k, e in errs.items():
        print(f"{k}: E_dev = {e:.4g}, E_O = {se.E_O_FREE[k]:.4g}, bound {se.free_bound(k):.4g}")
    bad = {k: (e, se.free_bound(k)) for k, e in errs.items() if not e <= se.free_bound(k)}
    assert not bad, bad


def test_free_variables_at_the_convention_points_are_the_oracles(free_runs):
    """x(q) on the bound itself, a derivative that overflows: the oracle's class, and zero where the oracle's gradient is zero"""
    _, sel, grads = free_runs["free_conventions"]
    _, want = se.oracle_free_gradient(sel)
    bad = [(case, float(se.FREE_CASES[case][i]), a, b) for case in sel for i, a, b in zip(sel[case], grads[case], want[case])
           if se.klass(a) != se.klass(b) or (b == 0.0 and a != 0.0)]
    assert not bad, bad
