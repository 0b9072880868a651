"""PSIS-LOO on the host: the NumPy restatement (tests/psis_reference.py) is PSIS, its direct and streaming forms agree, and
pymc_amd/csrc/psis.h -- the header k_psis_fold / k_psis_finish compile -- reproduces it.

`tests/psis_check.cpp` is a stand-alone program around the header (system compiler, -Wall -Wextra -Werror, address and
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
import psis_reference as pr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "psis_check.cpp")
INC = os.path.join(ROOT, "pymc_amd", "csrc")

S_LIST = [20, 21, 25, 26, 37, 64, 100, 203, 1000, 4000]


def test_tail_lengths():
    assert [pr.tail_len(S) for S in (20, 21, 37, 203, 1000, 4000)] == [4, 5, 8, 41, 95, 190]
    assert pr.tail_len(116000) + 1 <= 1024 < pr.tail_len(117000) + 1


@pytest.mark.parametrize("k", [0.2, 0.5, 0.9])
def test_the_restatement_recovers_the_shape_of_pareto_weights(k):
    # log-ratios Exp(mean k): ratios Pareto with shape k
    kh = []
    for seed in range(20):
        x = np.random.default_rng(1000 + seed).exponential(k, 4000)
        kh.append(pr.psis_direct(-x)[0])
    print("k", k, "mean khat", np.mean(kh))
    assert abs(np.mean(kh) - k) < 0.1


def _vectors(S, rng):
    """(label, values): random vectors of several spreads, vectors with duplicated draws, a constant vector"""
    out = []
    for scale in (0.05, 1.0, 4.0):
        out.append((f"normal*{scale}", -3.0 + scale * rng.standard_normal(S)))
    out.append(("heavy", -rng.exponential(0.8, S) * rng.exponential(1.0, S)))
    half = rng.standard_normal((S + 1) // 2)
    out.append(("duplicated", np.concatenate([half, half])[:S]))
    out.append(("few distinct", rng.integers(0, 7, S).astype("float64") * 0.37 - 2.0))
    out.append(("constant", np.full(S, -1.25)))
    return out


def _close(got, ref, tol, rel):
    if math.isnan(ref) or math.isinf(ref):
        return (math.isnan(got) and math.isnan(ref)) or got == ref
    return abs(got - ref) <= tol * (max(1.0, abs(ref)) if rel else 1.0)


def test_direct_and_streaming_forms_agree():
    worst_e = worst_k = 0.0
    for S in S_LIST:
        rng = np.random.default_rng(S)
        for label, ll in _vectors(S, rng):
            kd, ed = pr.psis_direct(ll)
            ks, es = pr.psis_streaming(ll)
            assert _close(ks, kd, 1e-12, False), (S, label, ks, kd)
            assert _close(es, ed, 1e-12, True), (S, label, es, ed)
            if math.isfinite(kd):
                worst_k = max(worst_k, abs(ks - kd))
            worst_e = max(worst_e, abs(es - ed) / max(1.0, abs(ed)))
    print("worst relative elpd difference", worst_e, "worst khat difference", worst_k)


def test_conventions_of_non_finite_values():
    ll = -np.abs(np.random.default_rng(3).standard_normal(37))
    for form in (pr.psis_direct, pr.psis_streaming):
        a = ll.copy(); a[11] = -np.inf
        assert form(a) == (math.inf, -math.inf)
        for bad in (np.nan, np.inf):
            a = ll.copy(); a[30] = bad
            assert all(math.isnan(v) for v in form(a))
            a[2] = -np.inf
            assert all(math.isnan(v) for v in form(a))


# ---- the header ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(INC, "psis.h")), "pymc_amd/csrc/psis.h is missing"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    out = str(tmp_path_factory.mktemp("psis") / "psis_check")
    base = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + INC, SRC, "-o", out]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return out


def _tok(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("inf" if v == math.inf else ("-inf" if v == -math.inf else v.hex()))


def _run(exe, cases):
    """cases: (ll, reff, stride, column) -> [(khat, elpd, m_rest, r_rest)]"""
    req = "".join(f"{len(ll)} {_tok(reff)} {stride} {col} " + " ".join(_tok(v) for v in ll) + "\n" for ll, reff, stride, col in cases)
    r = subprocess.run([exe], input=req, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = [float("nan") if w in ("nan", "-nan") else float.fromhex(w) if "x" in w else float(w) for w in r.stdout.split()]
    assert len(out) == 4 * len(cases)
    return [tuple(out[4 * i:4 * i + 4]) for i in range(len(cases))]


def _header_cases():
    cases = []
    for S in (20, 21, 37, 203, 1000):
        rng = np.random.default_rng(7 * S)
        M = pr.tail_len(S)
        for label, ll in _vectors(S, rng):
            cases.append((f"S={S} {label}", ll, 1.0, 1, 0))
        ll = -2.0 + 1.5 * rng.standard_normal(S)
        cases.append((f"S={S} stride 5", ll, 1.0, 5, 3))
        cases.append((f"S={S} reff 0.4", ll, 0.4, 2, 1))
        # ties at the cutoff: the (M + 1)-th smallest value repeated on both sides of the cut
        t = ll.copy()
        srt = np.argsort(t)
        t[srt[M - 2:M + 3]] = t[srt[M]]
        cases.append((f"S={S} ties at the cutoff", t, 1.0, 3, 2))
        a = ll.copy(); a[S // 3] = -np.inf
        cases.append((f"S={S} -inf draw", a, 1.0, 2, 0))
        a = ll.copy(); a[rng.random(S) < 0.5] = -np.inf       # more of them than the column keeps: some are rejected, some evicted
        cases.append((f"S={S} -inf at half the draws", a, 1.0, 1, 0))
        a[S // 2 + 1] = np.nan
        cases.append((f"S={S} -inf at half the draws and a NaN", a, 1.0, 1, 0))
        a = ll.copy(); a[S - 2] = np.nan
        cases.append((f"S={S} NaN draw", a, 1.0, 2, 1))
        a = ll.copy(); a[1] = np.nan
        cases.append((f"S={S} early NaN draw", a, 1.0, 1, 0))
        a = ll.copy(); a[S // 2] = np.inf
        cases.append((f"S={S} +inf draw", a, 1.0, 1, 0))
    return cases


def test_the_header_reproduces_the_restatement(exe):
    cases = _header_cases()
    got = _run(exe, [c[1:] for c in cases])
    worst_e = worst_k = 0.0
    for (label, ll, reff, _, _), (khat, elpd, m_rest, r_rest) in zip(cases, got):
        kd, ed = pr.psis_direct(ll, reff)
        assert _close(khat, kd, 1e-12, False), (label, khat, kd)
        assert _close(elpd, ed, 1e-12, True), (label, elpd, ed)
        if math.isfinite(kd):
            worst_k = max(worst_k, abs(khat - kd))
        if math.isfinite(ed):
            worst_e = max(worst_e, abs(elpd - ed) / max(1.0, abs(ed)))
        # the running pair is the restatement's, to rounding of exp (the host's libm on both sides: bit for bit here)
        _, m_ref, r_ref = pr.fold(ll, reff)
        assert m_rest == m_ref and (r_rest == r_ref or (math.isnan(r_rest) and math.isnan(r_ref))), (label, m_rest, m_ref, r_rest, r_ref)
    print("header: worst relative elpd difference", worst_e, "worst khat difference", worst_k)


def test_the_program_refuses_malformed_input(exe):
    assert subprocess.run([exe], input="20 1.0 1 0 0x1p0\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="20 1.0 2 2\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="3 1.0x\n", capture_output=True, text=True).returncode == 2


# ---- the host arithmetic of `az.loo` and the refusals -----------------------------------------------------------------------------
def test_loo_from_pointwise_is_arviz_loo_on_the_log_scale():
    from pymc_amd import loglik

    rng = np.random.default_rng(4)
    S, N = 203, 17
    ll = rng.normal(size=(S, N)) * 1.5 - 3.0
    khat, elpd_i, lppd_i = pr.psis_matrix(ll)
    out = loglik.loo_from_pointwise(elpd_i, khat, lppd_i, S, pointwise=True)
    assert out["elpd_loo"] == float(elpd_i.sum()) and out["p_loo"] == float(lppd_i.sum() - elpd_i.sum())
    np.testing.assert_allclose(out["se"], math.sqrt(N * np.var(elpd_i)), rtol=1e-15)
    assert out["n_samples"] == S and out["n_data_points"] == N
    assert out["good_k"] == pr.good_k(S) == min(1.0 - 1.0 / math.log10(S), 0.7) and out["good_k"] < 0.7
    assert loglik.loo_from_pointwise(elpd_i, khat, lppd_i, 4000)["good_k"] == 0.7
    assert out["warning"] is bool(np.any(khat > pr.good_k(S)))
    assert loglik.loo_from_pointwise(elpd_i, np.full(N, 0.1), lppd_i, S)["warning"] is False
    assert loglik.loo_from_pointwise(elpd_i, np.where(np.arange(N) == 3, np.inf, 0.1), lppd_i, S)["warning"] is True
    assert np.array_equal(out["loo_i"], elpd_i) and np.array_equal(out["pareto_k"], khat)
    assert set(loglik.loo_from_pointwise(elpd_i, khat, lppd_i, S)) == {"elpd_loo", "se", "p_loo", "n_samples", "n_data_points", "warning", "good_k"}
    assert out["p_loo"] > 0.0          # leaving an observation out lowers its predictive density


def test_loo_refuses_what_waic_refuses():
    from pymc_amd import loglik, models
    from pymc_amd.model_spec import ModelBuilder

    def both(exc, match, spec, **kw):
        for fn in (loglik.waic, loglik.loo):
            with pytest.raises(exc, match=match):
                fn(spec, np.zeros((1, 2, spec.n)), **kw)

    both(ValueError, "another step method", models.normal_mixture(N=50, K=3), var_name="y|c")
    cond = models.normal_mixture(N=50, K=3, form="node")
    cond.extra = {}
    both(ValueError, "conditional mixture", cond)
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0)
    m.Normal("y1", a, 1.0, observed=np.zeros(3))
    m.Normal("y2", a, 2.0, observed=np.ones(4))
    two = m.build()
    both(TypeError, "var_name cannot be None", two)
    both(KeyError, "not observed", two, var_name="a")
    both(ValueError, "no observed variable", models.std_normal())
    for fn in (loglik.waic, loglik.loo):
        with pytest.raises(ValueError, match="raveled unconstrained"):
            fn(two, np.zeros((1, 2, two.n + 1)), var_name="y1")


def test_the_calls_refuse_a_null_handle():
    import ctypes as C

    import __graft_entry__ as g

    g.build_engine()
    from pymc_amd import _lib

    lib = _lib.load()
    out = np.full(4, 7.0)
    n = C.c_int64(-1)
    assert not lib.nuts_psis_create(None, 0, 0, 100, 1.0)
    assert lib.nuts_psis_update(None, _lib.dptr(out), 1) == _lib.NUTS_E_ARG
    assert lib.nuts_psis_read(None, None, None, None, C.byref(n)) == _lib.NUTS_E_ARG and n.value == -1
    assert lib.nuts_psis_read_raw(None, _lib.dptr(out), _lib.dptr(out), C.byref(n)) == _lib.NUTS_E_ARG and n.value == -1
    lib.nuts_psis_destroy(None)
    assert np.all(out == 7.0)
