"""The convergence summary on the device (csrc/summary.h, csrc/summary_kernel.h, pymc_amd/summary.py) against the NumPy restatement
(tests/summary_reference.py), which tests/test_summary_host.py pins to pymc_amd/stats.py and to closed forms.

Bars: the HDI and the NaN pattern `array_equal`; mean and sd 1e-12 relative; r_hat 1e-10; ESS and MCSE columns 1e-9 relative (the
project's device bars).  The HDI ends are draws, and the indicator sets behind ess_tail are those of the restatement by
construction: the pooled quantile equals a draw only when the interpolation weight is 0 or its two ends are equal, and both cases
are exact under NumPy's formula, which summary.h follows operation by operation.  Everything about blocks, neighbours and the order
of the columns is `array_equal`.
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import summary_reference as sr  # noqa: E402
from pymc_amd import _lib, models, stats, summary  # noqa: E402

pytestmark = pytest.mark.gpu

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stats_kat.npz")
KAT_NAMES = ("iid", "ar1", "anti", "shifted", "drift", "ties")
REL = {"mean": 1e-12, "sd": 1e-12, "mcse_mean": 1e-9, "mcse_sd": 1e-9, "ess_bulk": 1e-9, "ess_tail": 1e-9}


def _columns(C, N, P, seed):
    """(C, N, P): the ten kinds of tests/summary_reference.py, again with other seeds until P columns are there"""
    cols = []
    while len(cols) < P:
        cols += [x for _, x in sr.kinds(C, N, seed + len(cols))]
    return np.stack(cols[:P], axis=2)


def _hold(label, got, ref):
    for k in sr.COLUMNS:
        g, r = got[k], ref[k]
        assert g.shape == r.shape, (label, k)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, k, g, r)
        ok = ~np.isnan(r)
        if k in ("hdi_lo", "hdi_hi"):
            worst = float(np.abs(g[ok] - r[ok]).max()) if ok.any() else 0.0
            print(f"{label}: {k} worst absolute difference {worst:.3e}")
            assert np.array_equal(g, r, equal_nan=True), (label, k, g, r)
        elif k == "r_hat":
            worst = float(np.abs(g[ok] - r[ok]).max()) if ok.any() else 0.0
            print(f"{label}: {k} worst absolute difference {worst:.3e}")
            assert worst <= 1e-10, (label, k, g, r)
        else:
            err = np.abs(g[ok] - r[ok]) / np.where(r[ok] == 0.0, 1.0, np.abs(r[ok]))
            worst = float(err.max()) if ok.any() else 0.0
            print(f"{label}: {k} worst relative difference {worst:.3e}")
            assert worst <= REL[k], (label, k, g, r)


def _hold_stats_py(label, x, got):
    """ess_bulk and r_hat against the benchmark's own estimators, for the columns they are defined on"""
    fin = np.all(np.isfinite(x), axis=(0, 1))
    if x.shape[1] // 2 < 4 or not fin.any():
        return
    with np.errstate(all="ignore"):
        e, r = stats.ess_bulk_many(x[:, :, fin]), stats.rhat_many(x[:, :, fin])
    ge, gr = got["ess_bulk"][fin], got["r_hat"][fin]
    assert np.array_equal(np.isnan(gr), np.isnan(r)), label
    ok = ~np.isnan(r)
    print(f"{label}: vs stats.py ess_bulk {float(np.abs(ge / e - 1.0).max()):.3e} r_hat {float(np.abs(gr[ok] - r[ok]).max()) if ok.any() else 0.0:.3e}")
    assert np.all(np.abs(ge - e) <= 1e-9 * np.abs(e)) and np.all(np.abs(gr[ok] - r[ok]) <= 1e-9 * np.abs(r[ok])), label


@pytest.fixture(scope="module")
def small():
    """{(C, N): (x, device summary, restatement)} of the small shapes at P = 65, computed once"""
    out = {}
    for C, N in ((1, 8), (2, 9), (3, 101), (4, 100), (1, 7)):
        x = _columns(C, N, 65, 1000 * C + N)
        out[(C, N)] = (x, summary.summarize(x, device=0), sr.summarize(x))
    return out


@pytest.mark.parametrize("shape", [(1, 8), (2, 9), (3, 101), (4, 100), (1, 7)])
def test_every_column_against_the_restatement(small, shape):
    x, got, ref = small[shape]
    _hold(f"{shape} P=65", got, ref)
    _hold_stats_py(f"{shape} P=65", x, got)
    if shape == (1, 7):   # N // 2 = 3: no ESS and no MCSE, everything else as usual
        fin = np.all(np.isfinite(x), axis=(0, 1))
        assert np.all(np.isnan(got["ess_bulk"])) and np.all(np.isnan(got["mcse_sd"])) and np.all(np.isfinite(got["hdi_lo"][fin]))


@pytest.mark.parametrize("C,N,P,pick", [(8, 1000, 3, (1, 3, 5)), (8, 1024, 2, (2, 6))])
def test_long_traces_up_to_the_limit(C, N, P, pick):
    """8 x 1000 (the second benchmark configuration) and 8 x 1024 = max_draws(): AR 0.9, a random walk (its scans run to the last
    lag) and values with ties; AR -0.5 and Cauchy draws at the limit"""
    assert summary.max_draws() == 8192
    kinds = sr.kinds(C, N, C + N)
    x = np.stack([kinds[i][1] for i in pick], axis=2)
    got = summary.summarize(x, device=0)
    _hold(f"{C}x{N} {[kinds[i][0] for i in pick]}", got, sr.summarize(x))
    _hold_stats_py(f"{C}x{N}", x, got)


def test_a_trace_above_the_limit_is_refused():
    lib = _lib.load()
    limit = summary.max_draws()
    x = np.zeros((1, limit + 1, 1))
    with pytest.raises(ValueError, match=f"{limit}.*out of scope"):
        summary.summarize(x, device=0)
    out = np.full((9, 1), 7.0)
    assert lib.nuts_summary(_lib.dptr(x), 1, limit + 1, 1, 0.94, _lib.dptr(out)) == _lib.NUTS_E_ARG
    assert str(limit) in _lib.last_error() and np.all(out == 7.0)


@pytest.mark.parametrize("name", KAT_NAMES)
def test_the_known_answers(name):
    k = np.load(KAT)
    x = k[name + "_x"]
    got = summary.summarize(x, device=0)
    _hold("kat " + name, got, sr.summarize(x))
    assert abs(got["ess_bulk"][0] - float(k[name + "_ess_bulk"])) <= 1e-9 * float(k[name + "_ess_bulk"])
    assert abs(got["r_hat"][0] - float(k[name + "_rhat"])) <= 1e-10


def test_hdi_prob():
    x = _columns(3, 101, 7, 5)
    for prob in (0.5, 0.05, 0.9999):
        got, ref = summary.summarize(x, hdi_prob=prob, device=0), sr.summarize(x, prob)
        for k in ("hdi_lo", "hdi_hi"):
            assert np.array_equal(got[k], ref[k], equal_nan=True), (prob, k)


def _same(a, b, idx=None):
    return all(np.array_equal(a[k] if idx is None else a[k][idx], b[k], equal_nan=True) for k in sr.COLUMNS)


def test_a_row_depends_on_its_own_draws_only(small):
    x, got, _ = small[(3, 101)]
    try:
        for block in (1, 7):
            _lib.set_engine_option("NUTS_SUMMARY_BLOCK", block)
            assert _same(summary.summarize(x, device=0), got), block
    finally:
        _lib.unset_engine_option("NUTS_SUMMARY_BLOCK")
    assert _same(got, summary.summarize(x[:, :, :7], device=0), slice(0, 7))
    for p in (0, 6, 33, 64):
        assert _same(got, summary.summarize(x[:, :, p], device=0), slice(p, p + 1)), p
    perm = np.random.default_rng(0).permutation(65)
    assert _same(got, summary.summarize(x[:, :, perm], device=0), perm)


# ---- the public interface ------------------------------------------------------------------------------------------------------
def test_summary_of_a_model_and_sample_with_summary():
    from pymc_amd.sampling import sample

    spec = models.eight_schools()
    res = sample(draws=50, tune=50, chains=2, model=spec, random_seed=23, device=0, summary=True)
    plain = sample(draws=50, tune=50, chains=2, model=spec, random_seed=23, device=0)
    try:
        assert "summary" not in plain and np.array_equal(plain["draws"], res["draws"])
        out = summary.summary(spec, res, device=0)
        assert out["names"] == [f"eta[{i}]" for i in range(8)] + ["mu", "tau"]
        assert list(out) == ["names", *sr.COLUMNS] and all(out[k].shape == (10,) for k in sr.COLUMNS)
        assert res["summary"]["names"] == out["names"] and _same(res["summary"], out)
        tau = summary.summarize(np.exp(res["draws"][:, :, 9]), device=0)
        assert _same(out, tau, slice(9, 10))
        _hold("eight schools", {k: out[k] for k in sr.COLUMNS}, sr.summarize(np.concatenate([res["draws"][:, :, :9], np.exp(res["draws"][:, :, 9:])], axis=2)))
        sub = summary.summary(spec, res["draws"], var_names=["tau", "mu", "tau_log__"], include_transformed=True, device=0)
        assert sub["names"] == ["mu", "tau_log__", "tau"] and _same(out, {k: sub[k][[0, 2]] for k in sr.COLUMNS}, [8, 9])
    finally:
        res["step"].close()
        plain["step"].close()
