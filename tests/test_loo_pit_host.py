"""LOO-PIT on the host: the NumPy restatement (tests/loo_pit_reference.py) weights like PSIS, does not depend on the order of the
draws and is calibrated where the posterior p-value is not; psis_fit / psis_weight of pymc_amd/csrc/psis.h -- the header
k_psis_fit / k_loo_weight compile -- reproduce its weights when fed draw by draw.

`tests/loo_pit_check.cpp` is a stand-alone program around the header (system compiler, -Wall -Wextra -Werror, address and
undefined-behaviour sanitizers when they link); it is never loaded into Python.
"""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loo_pit_reference as lr  # noqa: E402
import psis_reference as pr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "loo_pit_check.cpp")
INC = os.path.join(ROOT, "pymc_amd", "csrc")
S_LIST = (20, 21, 37, 203, 1000)


def _direct_weights(ll, reff=1.0):
    """psis_direct's own weights: its arithmetic, returning exp(w) instead of the elpd"""
    return lr.psis_weights(ll, reff, tie_mean=False)


def test_without_ties_the_weights_are_psis_directs_own():
    for S in S_LIST:
        rng = np.random.default_rng(11 * S)
        for scale in (0.05, 1.0, 4.0):
            ll = -3.0 + scale * rng.standard_normal(S)
            assert np.unique(ll).size == S
            w = lr.psis_weights(ll)
            assert np.array_equal(w, _direct_weights(ll))
            # ... and psis_direct's elpd is the log of the weighted mean of exp(ll) under them
            khat, elpd = pr.psis_direct(ll)
            np.testing.assert_allclose(math.log(np.sum(w * np.exp(ll - ll.max()))) + ll.max(), elpd, rtol=1e-13, atol=1e-13)
            assert abs(w.sum() - 1.0) <= 1e-14


def _tied(S, rng, scale=1.0):
    """a fifth of the draws duplicated at random places"""
    ll = -3.0 + scale * rng.standard_normal(S)
    dup = rng.choice(S, S // 5, replace=False)
    ll[dup] = ll[rng.choice(np.setdiff1d(np.arange(S), dup), S // 5)]
    return ll


def test_under_ties_the_pit_does_not_depend_on_the_order_of_the_draws():
    moved_argsort = 0.0
    for S in S_LIST:
        rng = np.random.default_rng(13 * S)
        ll = _tied(S, rng, 2.0)
        assert np.unique(ll).size < S
        y_rep = rng.standard_normal(S)
        a = lr.loo_pit_vector(ll, y_rep, 0.3)
        a0 = lr.loo_pit_vector(ll, y_rep, 0.3, tie_mean=False)
        assert abs(a["sum_w"] - 1.0) <= 1e-14
        for _ in range(3):
            perm = rng.permutation(S)
            b = lr.loo_pit_vector(ll[perm], y_rep[perm], 0.3)
            for k in lr.COLUMNS:
                np.testing.assert_allclose(b[k], a[k], rtol=1e-12, atol=1e-13, err_msg=f"S={S} {k}")
            b0 = lr.loo_pit_vector(ll[perm], y_rep[perm], 0.3, tie_mean=False)
            moved_argsort = max(moved_argsort, abs(b0["p_lt"] - a0["p_lt"]))
    print("argsort rule: the PIT moved by up to", moved_argsort, "under a permutation of the draws")
    assert moved_argsort > 1e-6          # (the rule the restatement replaces does depend on the order)


def test_non_finite_values_give_nan():
    ll = -np.abs(np.random.default_rng(3).standard_normal(37))
    y_rep = np.random.default_rng(4).standard_normal(37)
    for bad in (-np.inf, np.nan, np.inf):
        a = ll.copy(); a[11] = bad
        assert all(math.isnan(v) for v in lr.loo_pit_vector(a, y_rep, 0.0).values())
    # a NaN replicate: the moments of its observation, never the weighted counts
    y = y_rep.copy(); y[5] = np.nan
    got, ref = lr.loo_pit_vector(ll, y, 0.0), lr.loo_pit_vector(np.delete(ll, 5), np.delete(y, 5), 0.0)
    assert math.isnan(got["loo_mean"]) and math.isnan(got["loo_sd"]) and got["sum_w"] == pytest.approx(1.0, abs=1e-14)
    assert 0.0 < got["p_lt"] < 1.0 and got["p_eq"] == 0.0 and ref["p_lt"] > 0.0


def _ks_uniform(p):
    srt, n = np.sort(p), p.size
    return max(np.max(np.arange(1, n + 1) / n - srt), np.max(srt - np.arange(n) / n))


def test_loo_pit_is_calibrated():
    """y_i ~ N(0, 1), i < 500; mu ~ N(0, 1), y_i | mu ~ N(mu, 1): mu | y ~ N(sum y / (n + 1), 1 / (n + 1)); S = 1000 draws of it and
    one replicate of every observation per draw.  Both assertions are on the restatement alone."""
    rng = np.random.default_rng(500)
    N, S = 500, 1000
    y = rng.standard_normal(N)
    mu = y.sum() / (N + 1.0) + rng.standard_normal(S) / math.sqrt(N + 1.0)
    ll = -0.5 * (y[None, :] - mu[:, None]) ** 2 - 0.5 * math.log(2.0 * math.pi)
    y_rep = mu[:, None] + rng.standard_normal((S, N))
    ref = lr.loo_pit_matrix(ll, y_rep, y)
    pit = ref["p_lt"] + ref["p_eq"]
    assert np.all(np.abs(ref["sum_w"] - 1.0) <= 1e-13) and np.all((pit >= 0.0) & (pit <= 1.0))
    ks = _ks_uniform(pit)
    p_post = np.mean(y_rep < y[None, :], axis=0)
    print("sup |ECDF(loo_pit) - uniform|", ks, "bar", 1.95 / math.sqrt(N), "var of the posterior p-values", p_post.var(), "of the LOO-PIT", pit.var())
    assert ks <= 1.95 / math.sqrt(N)
    assert p_post.var() < 1.0 / 12.0


def test_loo_pit_is_calibrated_where_the_posterior_p_value_visibly_is_not():
    """The same model fitted per GROUP of 2 observations (250 groups, each its own mu): an observation is half of the data its
    replicate was fitted to, so the posterior p-values pile up at 1/2 far more than one observation in 500 can make them."""
    rng = np.random.default_rng(2024)
    N, S, g = 500, 1000, 2
    y = rng.standard_normal(N)
    yg = y.reshape(-1, g)
    post_mean = yg.sum(axis=1) / (g + 1.0)
    mu = post_mean[None, :] + rng.standard_normal((S, N // g)) / math.sqrt(g + 1.0)     # [S][groups]
    mu_i = np.repeat(mu, g, axis=1)                                                    # [S][N]
    ll = -0.5 * (y[None, :] - mu_i) ** 2 - 0.5 * math.log(2.0 * math.pi)
    y_rep = mu_i + rng.standard_normal((S, N))
    ref = lr.loo_pit_matrix(ll, y_rep, y)
    pit = ref["p_lt"] + ref["p_eq"]
    assert np.all(np.abs(ref["sum_w"] - 1.0) <= 1e-13) and np.all((pit >= 0.0) & (pit <= 1.0))
    ks = _ks_uniform(pit)
    p_post = np.mean(y_rep < y[None, :], axis=0)
    print("groups of 2: sup |ECDF(loo_pit) - uniform|", ks, "of the posterior p-values", _ks_uniform(p_post), "bar", 1.95 / math.sqrt(N),
          "var of the posterior p-values", p_post.var())
    assert ks <= 1.95 / math.sqrt(N)
    assert p_post.var() < 1.0 / 12.0


# ---- the header ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(INC, "psis.h")), "pymc_amd/csrc/psis.h is missing"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    out = str(tmp_path_factory.mktemp("loo_pit") / "loo_pit_check")
    base = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + INC, SRC, "-o", out]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return out


def _tok(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("inf" if v == math.inf else ("-inf" if v == -math.inf else v.hex()))


def _num(w):
    return float("nan") if w in ("nan", "-nan") else float.fromhex(w) if "x" in w else float(w)


def _run(exe, cases):
    """cases: (ll, reff, stride, column, extra values) -> [(record: state khat elpd c xc tl sigma logden, weights [S + Q])]"""
    req = "".join(f"{len(ll)} {_tok(reff)} {stride} {col} " + " ".join(_tok(v) for v in ll) + f" {len(extra)} " + " ".join(_tok(v) for v in extra) + "\n"
                  for ll, reff, stride, col, extra in cases)
    r = subprocess.run([exe], input=req, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    out = []
    for ln, (ll, _, _, _, extra) in zip(lines, cases):
        v = [_num(w) for w in ln.split()]
        assert len(v) == 8 + len(ll) + len(extra)
        out.append((v[:8], np.array(v[8:])))
    return out


def _header_cases():
    cases = []
    for S in S_LIST:
        rng = np.random.default_rng(17 * S)
        for scale in (0.05, 1.0, 4.0):
            cases.append((f"S={S} normal*{scale}", -3.0 + scale * rng.standard_normal(S), 1.0, 1, 0))
            cases.append((f"S={S} a fifth duplicated *{scale}", _tied(S, rng, scale), 1.0, 3, 1))
        half = rng.standard_normal((S + 1) // 2)
        cases.append((f"S={S} every draw twice", np.concatenate([half, half])[:S], 1.0, 2, 0))
        cases.append((f"S={S} few distinct", rng.integers(0, 7, S).astype("float64") * 0.37 - 2.0, 1.0, 1, 0))
        cases.append((f"S={S} constant", np.full(S, -1.25), 1.0, 1, 0))
        ll = -2.0 + 1.5 * rng.standard_normal(S)
        cases.append((f"S={S} stride 5", ll, 1.0, 5, 3))
        cases.append((f"S={S} reff 0.4", ll, 0.4, 2, 1))
        M = pr.tail_len(S)
        t = ll.copy()
        srt = np.argsort(t)
        t[srt[M - 2:M + 3]] = t[srt[M]]
        cases.append((f"S={S} ties at the cutoff", t, 1.0, 3, 2))
        for bad, where in ((-np.inf, S // 3), (np.nan, S - 2), (np.inf, S // 2)):
            a = ll.copy(); a[where] = bad
            cases.append((f"S={S} a {bad} draw", a, 1.0, 2, 1))
    return cases


def test_the_header_fed_draw_by_draw_reproduces_the_restatement(exe):
    cases = _header_cases()
    got = _run(exe, [(ll, reff, stride, col, ()) for _, ll, reff, stride, col in cases])
    worst = worst_sum = 0.0
    for (label, ll, reff, _, _), (rec, w) in zip(cases, got):
        ref = lr.psis_weights(ll, reff)
        state = int(rec[0])
        if np.any(np.isnan(ref)):
            assert state == (1 if np.any(ll == -np.inf) and not (np.any(np.isnan(ll)) or np.any(ll == np.inf)) else 2), (label, state)
            assert np.all(np.isnan(w)), label
            continue
        assert state == 0, (label, state)
        assert ll.max() - ll.min() < 600.0
        rel = float(np.max(np.abs(w - ref) / ref))
        worst, worst_sum = max(worst, rel), max(worst_sum, abs(float(np.sum(w)) - 1.0))
        assert rel <= 1e-12, (label, rel)
        assert abs(float(np.sum(w)) - 1.0) <= 1e-12, (label, float(np.sum(w)))
        # the record is psis_finish's fit
        kd, ed = pr.psis_direct(ll, reff)
        assert (rec[1] == kd) or abs(rec[1] - kd) <= 1e-12, (label, rec[1], kd)
        assert abs(rec[2] - ed) <= 1e-12 * max(1.0, abs(ed)), (label, rec[2], ed)
    print("header: worst relative weight difference", worst, "worst |sum w - 1|", worst_sum)


def test_a_value_the_first_pass_did_not_see_takes_its_insertion_rank(exe):
    rng = np.random.default_rng(5)
    ll = -2.0 + 1.5 * rng.standard_normal(203)
    srt = np.sort(ll)
    M = pr.tail_len(203)
    extra = [srt[0] - 1.0, 0.5 * (srt[3] + srt[4]), 0.5 * (srt[M - 1] + srt[M]), srt[-1] + 1.0]
    (rec, w), = _run(exe, [(ll, 1.0, 1, 0, extra)])
    by_rank = w[:203][np.argsort(ll)]
    we = w[203:]
    assert int(rec[5]) == M
    assert we[0] == by_rank[0] and we[1] == by_rank[4] and we[2] == by_rank[M - 1]
    np.testing.assert_allclose(we[3], math.exp(-(srt[-1] + 1.0) - rec[3] - rec[7]), rtol=1e-15)
    assert np.all(np.isfinite(we))


def test_the_program_refuses_malformed_input(exe):
    assert subprocess.run([exe], input="20 1.0 1 0 0x1p0\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="20 1.0 2 2\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="2 1.0 1 0 -1 -2 -1\n", capture_output=True, text=True).returncode == 2


# ---- the host arithmetic of `predictive.loo_pit` ------------------------------------------------------------------------------------
def test_loo_pit_from_accumulators():
    from pymc_amd import predictive

    rng = np.random.default_rng(8)
    S, N = 203, 9
    ll = rng.normal(size=(S, N)) * 1.5 - 3.0
    ll[7, 2] = -np.inf
    y_rep, y = rng.normal(size=(S, N)).round(1), rng.normal(size=N).round(1)
    ref = lr.loo_pit_matrix(ll, y_rep, y)
    khat, elpd_i, lppd_i = pr.psis_matrix(ll)
    sum_w2 = 1.0 / ref["ess"]
    out = predictive.loo_pit_from_accumulators(ref["p_lt"], ref["p_eq"], ref["loo_mean"], ref["loo_sd"] ** 2, ref["sum_w"], sum_w2, elpd_i, khat, lppd_i, S)
    assert np.array_equal(out["loo_pit"], ref["p_lt"] + ref["p_eq"], equal_nan=True)
    assert np.array_equal(out["loo_pit_mid"], ref["p_lt"] + 0.5 * ref["p_eq"], equal_nan=True)
    np.testing.assert_allclose(out["loo_sd"], ref["loo_sd"], rtol=1e-15)
    np.testing.assert_allclose(out["ess"], ref["ess"], rtol=1e-15)
    assert np.isnan(out["loo_pit"][2]) and np.isnan(out["ess"][2]) and out["loo_i"][2] == -np.inf and out["pareto_k"][2] == np.inf
    assert np.array_equal(out["pareto_k"], khat) and np.array_equal(out["loo_i"], elpd_i)
    assert set(predictive.loglik.loo_from_pointwise(elpd_i, khat, lppd_i, S)) < set(out)
    assert "loo_i" not in predictive.loo_pit_from_accumulators(ref["p_lt"], ref["p_eq"], ref["loo_mean"], ref["loo_sd"] ** 2, ref["sum_w"], sum_w2,
                                                              elpd_i, khat, lppd_i, S, pointwise=False)
    bad = ref["sum_w"].copy()
    bad[4] = 0.93
    with pytest.raises(ValueError, match="the second pass did not see the draws of the first"):
        predictive.loo_pit_from_accumulators(ref["p_lt"], ref["p_eq"], ref["loo_mean"], ref["loo_sd"] ** 2, bad, sum_w2, elpd_i, khat, lppd_i, S)
    bad = ref["sum_w"].copy()
    bad[4] = np.nan
    with pytest.raises(ValueError, match="the second pass did not see"):
        predictive.loo_pit_from_accumulators(ref["p_lt"], ref["p_eq"], ref["loo_mean"], ref["loo_sd"] ** 2, bad, sum_w2, elpd_i, khat, lppd_i, S)


def test_loo_pit_refuses_what_the_two_passes_refuse():
    from pymc_amd import models, predictive
    from pymc_amd.model_spec import ModelBuilder

    with pytest.raises(ValueError, match="another step method"):
        predictive.loo_pit(models.normal_mixture(N=50, K=3), np.zeros((1, 2, models.normal_mixture(N=50, K=3).n)), var_name="y|c")
    with pytest.raises(ValueError, match="no observed variable"):
        predictive.loo_pit(models.std_normal(), np.zeros((1, 2, models.std_normal().n)))
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    m.Normal("y1", a, 1.0, observed=np.zeros(3))
    m.Normal("y2", a, 2.0, observed=np.ones(4))
    two = m.build()
    with pytest.raises(TypeError, match="var_name cannot be None"):
        predictive.loo_pit(two, np.zeros((1, 2, two.n)))
    with pytest.raises(KeyError, match="not observed"):
        predictive.loo_pit(two, np.zeros((1, 2, two.n)), var_name="a")
    with pytest.raises(ValueError, match="raveled unconstrained"):
        predictive.loo_pit(two, np.zeros((1, 2, two.n + 1)), var_name="y1")


def test_the_calls_refuse_a_null_handle():
    import ctypes as C

    import __graft_entry__ as g

    g.build_engine()
    from pymc_amd import _lib

    lib = _lib.load()
    out = np.full(4, 7.0)
    n = C.c_int64(-1)
    assert not lib.nuts_loo_pit_create(None, 0)
    assert lib.nuts_loo_pit_update(None, _lib.dptr(out), 1, 0) == _lib.NUTS_E_ARG
    assert lib.nuts_loo_pit_read(None, None, None, None, None, None, None, C.byref(n)) == _lib.NUTS_E_ARG and n.value == -1
    lib.nuts_loo_pit_destroy(None)
    assert np.all(out == 7.0)
