"""The point table, truths and regimes of tests/logit_edges.py, and the oracle held to them, on the host.

The oracle's rows -- the gcc loop `oracle_logit_rows` through oracle/c_logit.py and the NumPy rows `ref_models._logit_rows` -- are
evaluated element by element on a model of one row and measured against mpmath: their error per regime IS the tabulated E_O
(asserted from both sides, so the tables cannot go stale).  The isolating model the device test reads its residuals from is checked
on both: the oracle's gradient element of mu_d equals the single row's residual bit for bit.
"""
import math
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logit_edges as le  # noqa: E402
import scalar_edges as se  # noqa: E402

from oracle import ref_models  # noqa: E402


def _c_oracle():
    from oracle import c_logit          # (loads oracle/_build/liboracle.so where it is used: a missing build is an error)

    return c_logit


def test_the_table_is_finite_signed_and_has_its_edges():
    eta = le.ETA
    assert np.all(np.isfinite(eta)) and len(set(eta.tolist())) == len(eta) and 600 <= len(eta) <= 1200
    have = set(eta.tolist())
    for v in (0.0, 5e-324, 2.0 ** -1022, 2.0 ** -53, 0.5 * le.LN2, 1074.5 * le.LN2, 1082 * le.LN2, 36.7368, 708.3964, 745.13, 750.0, 1e300):
        for s in (1.0, -1.0):
            for w in (np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)):
                assert float(s * w) + 0.0 in have, (s, w)
    assert not any(math.copysign(1.0, v) < 0 and v == 0 for v in eta)          # one zero


def test_the_truths_are_stable_and_every_regime_has_points():
    seen = {}
    for y in le.YS:
        for eta in le.ETA:
            lp, r, dr = le.truth(y, float(eta))          # (asserts: the same doubles at twice the precision)
            assert lp <= 0 and dr <= 0 and (r >= 0 if y else r <= 0)
            k = le.regime_of(y, float(eta))
            seen[k] = seen.get(k, 0) + 1
    assert set(seen) == set(le.REGIMES), sorted(set(le.REGIMES) ^ set(seen))
    assert min(seen.values()) >= 10, seen
    assert set(le.E_O) == {f"{k}/{o}" for k in le.REGIMES for o in le.OUTPUTS}


def test_the_truths_against_their_definitions():
    """lp = log p(y | eta) from the definition, r = d lp / d eta and d r / d eta by central differences (1400 bits: exp(-745) = 2^-1075
    next to 1 is still resolved to 2^-300 of itself)"""
    with mp.workprec(1400):
        for eta in (0.0, 1e-17, -1e-8, 0.3, -0.3, 5.0, -36.7368, 37.43, 100.0, -700.0, 745.0, -745.0):
            x, h = mp.mpf(eta), mp.ldexp(1, -60)
            for y in le.YS:
                lp, r, dr = le._truth_mp(y, x)
                p = 1 / (1 + mp.exp(-x)) if y else 1 / (1 + mp.exp(x))
                assert abs(lp - mp.log(p)) <= mp.ldexp(1, -200) * abs(lp), (eta, y)
                num = (le._truth_mp(y, x + h)[0] - le._truth_mp(y, x - h)[0]) / (2 * h)
                assert abs(num - r) <= mp.ldexp(1, -100) * abs(r), (eta, y)
                num = (le._truth_mp(y, x + h)[1] - le._truth_mp(y, x - h)[1]) / (2 * h)
                assert abs(num - dr) <= mp.ldexp(1, -100) * abs(dr), (eta, y)


def test_the_measure_and_its_floor():
    lp, r, _ = le.truth(1, 40.0)
    # the cancelling regime: a result of 0 where the truth is exp(-40) is within one rounding of the larger operand
    assert le.cancelling(1, 40.0) and not le.cancelling(1, -40.0) and not le.cancelling(0, 40.0) and not le.cancelling(1, 0.0)
    assert le.measure(0.0, 1, 40.0, "r") < 1.0 and le.measure(0.0, 1, 40.0, "lp") < 1.0
    assert le.measure(-se.ulp(40.0), 1, 40.0, "lp") < 1.01
    # ... and nowhere else: the same miss at y = 0, eta = -40 (truth -exp(-40), no floor) is 1 / ulp(40) of what an ulp of eta moves
    assert le.measure(0.0, 0, -40.0, "lp") > 1e14 and le.measure(0.0, 0, -40.0, "r") > 1e14
    assert le.measure(float("nan"), 0, 1.0, "lp") == math.inf
    assert le.measure(se._to_double(lp), 1, 40.0, "lp") <= 0.5 and le.measure(se._to_double(r), 1, 40.0, "r") <= 0.5


@pytest.mark.parametrize("which", ["c", "numpy"])
def test_the_oracle_error_per_regime_is_the_tabulated_one(which):
    table = le.E_O_C if which == "c" else le.E_O_NUMPY
    got, where = le.regime_errors(le.oracle_values(which))
    assert set(got) == set(table), sorted(set(got) ^ set(table))
    for k, e in got.items():
        print(f"{which} {k}: E_O = {e:.4g} (table {table[k]:.4g}) worst at eta = {where[k][0]!r}")
        assert e <= table[k] <= 1.5 * e + 1.0, (k, e, table[k])
    assert all(le.E_O[k] == min(le.E_O_C[k], le.E_O_NUMPY[k]) for k in le.E_O)
    assert all(le.bound(k) <= 2.0 * le.FACTOR for k in le.E_O)          # no regime where the references themselves are far off


SHAPES = [(12, 130), (20, 60), (80, 90)]


@pytest.mark.parametrize("G,rpg", SHAPES)
@pytest.mark.parametrize("which", ["c", "numpy"])
def test_the_isolating_model_returns_single_rows_on_the_oracle(which, G, rpg):
    """grad[mu_d] of the oracle on the isolating model is the residual of the one-row model at eta_d, bit for bit"""
    pts = np.concatenate([le.ETA[:: max(1, len(le.ETA) // 60)], [0.0, 1e300, -1e300, 750.0, -5e-324]])
    single = le.oracle_values(which, pts)
    for y in le.YS:
        spec, idx = le.rows_model(G, rpg, y)
        X = spec.logit_rows.X
        assert X.shape == (G * rpg, le.D) and np.all(X[:, 0] == 1.0) and np.count_nonzero(X[:, 1:]) == le.NPROBE
        assert [int(np.flatnonzero(X[:, d])[0]) for d in range(1, le.D)] == idx.tolist() and np.all(spec.logit_rows.y[idx] == y)
        f = _c_oracle().CRowsSpecLogpGrad(spec) if which == "c" else ref_models.SpecLogpGrad(spec)
        for i, ch in enumerate(le.chunks(pts)):
            with np.errstate(all="ignore"):
                _, grad = f(le.rows_point(G, rpg, ch))
            want = single[(y, "r")][le.NPROBE * i: le.NPROBE * i + len(ch)]
            # (+ 0.0: the sign of a zero residual comes from the oracle's sums over the other rows' -0.0 products, not from the logistic)
            assert np.array_equal(le.read_residuals(grad, len(ch)) + 0.0, want + 0.0), (y, ch)


def test_the_probes_sit_where_the_tiles_end():
    places = le.probe_places(12, 130)
    assert {g for g, _ in places} >= {0, 11} and {r for _, r in places} == {0, 127, 128, 129}
    for G, rpg in SHAPES[1:]:
        places = le.probe_places(G, rpg)
        assert {g for g, _ in places} >= {0, G - 1} and {0, rpg - 1} <= {r for _, r in places}


def test_the_summed_truth_of_the_isolating_model_is_the_oracles():
    """`mp_rows_model_logp` (priors and rows in mpmath) against the NumPy oracle's log-density, to the oracle's own rounding"""
    G, rpg = 12, 130
    for y in le.YS:
        spec, idx = le.rows_model(G, rpg, y)
        f = ref_models.SpecLogpGrad(spec)
        for etas in ([0.0] * 7, [1.0, -1.0, 40.0, -40.0, 1e-8, 36.7368, -18.0]):
            q = le.rows_point(G, rpg, etas)
            total, den, tabs = le.mp_rows_model_logp(G, rpg, y, tuple(etas))
            lp, _ = f(q)
            assert abs(float(total) - lp) <= 1e-12 * float(tabs), (y, etas, float(total), lp)
            assert float(den) > 0 and float(tabs) >= abs(float(total))


def test_the_glm_models_isolate_on_the_oracle():
    pts = le.ETA[:: max(1, len(le.ETA) // 128)][: le.GLM_P]
    pts = np.concatenate([pts, np.zeros(le.GLM_P - len(pts))])
    single = le.oracle_values("numpy", pts)
    for y in le.YS:
        spec = le.glm_model(le.GLM_P, y)
        with np.errstate(all="ignore"):
            _, grad = ref_models.evaluate(spec, pts)
        assert np.array_equal(grad + 0.0, single[(y, "r")] + 0.0)
        one = le.glm_model(1, y)
        for k in (0, 17, 40):
            with np.errstate(all="ignore"):
                lp, g = ref_models.evaluate(one, pts[k: k + 1])
            assert lp == single[(y, "lp")][k] and g[0] == single[(y, "r")][k]
