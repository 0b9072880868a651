"""Model comparison on the host: the NumPy restatement (tests/compare_reference.py) solves the stacking problem at least as well as
ArviZ's own formulation, and pymc_amd/csrc/compare.h -- the header k_cmp_terms / k_cmp_stack_pass / k_cmp_bb compile and whose solver
nuts_compare_stacking runs -- reproduces it.

`tests/compare_check.cpp` is a stand-alone program around the header (system compiler, -Wall -Wextra -Werror, address and
undefined-behaviour sanitizers when they link); it is never loaded into Python.

Inputs: `compare_reference.grid()`, N in {1, 2, 63, 64, 65, 257, 1000, 4097} x K in {2, 3, 4, 8} x {close, dominant, deep, dup}.

Curvature.  lambda, the smallest eigenvalue of -H on the sum-zero directions at the optimum, is computed for every non-`dup` input; the
device test bounds |w - w_ref| by sqrt(2 gap / lambda) with it.  -H is the second-moment matrix of the N vectors q_i. = p_i. / d_i, so
on the K - 1 sum-zero directions it is singular whenever N < K - 1 (N = 1, 2 with K >= 3: lambda is 0 to rounding, the weights are
not unique, as for `dup`) and its smallest eigenvalue is still noisy at N of a few times K: measured here, lambda >= 0.01 holds at
every input with N >= 257 (smallest 0.0111), while `dominant` with K = 8 gives 0.0071 - 0.0085 at N = 63 .. 65.  The assertion is therefore made for N >= 257; below, lambda is only printed and enters the device test's bound as it
is (a bound above 1 asks nothing of the weights: there the objective decides).
"""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compare_reference as cr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "compare_check.cpp")
INC = os.path.join(ROOT, "pymc_amd", "csrc")


@pytest.fixture(scope="module")
def solved():
    """every input of the grid, solved once by the restatement: (N, K, kind) -> (e, w, f, gap, passes)"""
    out = {}
    for N, K, kind, seed in cr.grid():
        e = cr.make(N, K, seed, kind)
        e.setflags(write=False)
        out[(N, K, kind)] = (e,) + cr.solve(e)
    return out


def test_moments_of_a_small_case():
    e = np.array([[-1.0, -2.0, -1.5], [-0.5, -0.25, -3.0], [-2.0, -1.0, -1.0], [-1.0, -1.0, -0.5]])
    elpd, se, dse, best = cr.moments(e)
    assert best == 1 and np.array_equal(elpd, [-4.5, -4.25, -6.0]) and dse[best] == 0.0
    np.testing.assert_allclose(se[0], math.sqrt(4 * np.var(e[:, 0])), rtol=1e-15)
    np.testing.assert_allclose(dse[2], math.sqrt(4 * np.var(e[:, 1] - e[:, 2])), rtol=1e-15)


def test_the_restatement_reaches_the_certificate_on_every_input(solved):
    worst_passes, worst_gap = 0, 0.0
    for (N, K, kind), (e, w, f, gap, passes) in solved.items():
        assert gap <= 1e-10 and passes <= 64, (N, K, kind, gap, passes)
        assert np.all(w >= 0.0) and abs(w.sum() - 1.0) <= 1e-12
        assert abs(gap - cr.kkt_gap(e, w)) <= 1e-14 and abs(f - cr.objective(e, w)) <= 1e-12 * max(1.0, abs(f))
        worst_passes, worst_gap = max(worst_passes, passes), max(worst_gap, gap)
    print("restatement: most passes", worst_passes, "largest kkt_gap", worst_gap)
    assert worst_passes <= 18


def test_the_restatement_is_no_worse_than_arviz_slsqp(solved):
    worst = -math.inf
    for (N, K, kind), (e, w, f, gap, passes) in solved.items():
        ws, fs = cr.slsqp(e)
        worst = max(worst, (fs - f) / max(1.0, abs(f)))
        assert f >= fs - 1e-9 * max(1.0, abs(f)), (N, K, kind, f, fs)
        assert f <= fs + N * max(cr.kkt_gap(e, ws), 0.0) + 1e-9 * max(1.0, abs(f))      # (the certificate bounds what SLSQP could gain)
    print("largest (f_slsqp - f) / max(1, |f|):", worst)


def test_the_unshifted_form_underflows_where_the_shifted_one_does_not(solved):
    e, w, f, gap, _ = solved[(1000, 4, "deep")]
    with np.errstate(divide="ignore"):
        assert np.exp(e).min() == 0.0 and np.isneginf(np.log(np.exp(e) @ w)).any()      # rows of zeros: ArviZ's objective is -inf
    assert np.isfinite(f) and gap <= 1e-10


def test_curvature_at_the_optimum(solved):
    smallest = {}
    for (N, K, kind), (e, w, f, gap, passes) in solved.items():
        if kind == "dup":
            continue
        lam = cr.curvature(e, w)
        smallest[N] = min(smallest.get(N, math.inf), lam)
        if N >= 257:
            assert lam >= 0.01, (N, K, kind, lam)
        if N < K - 1:
            assert abs(lam) <= 1e-12, (N, K, kind, lam)
    print("smallest lambda per N:", smallest)


def test_bootstrap_variates_are_exponential():
    g = cr.bb_variates(3, np.arange(64)[:, None], np.arange(4000)[None, :])
    assert np.all(np.isfinite(g)) and np.all(g >= 0.0)
    assert abs(g.mean() - 1.0) < 0.01 and abs(g.var() - 1.0) < 0.03
    assert abs(np.corrcoef(g[0], g[1])[0, 1]) < 0.06          # the two halves of one block
    # replicate b at observation i is a function of (seed, b, i) alone
    assert np.array_equal(cr.bb_variates(3, 5, np.arange(10)), g[5, :10]) and not np.array_equal(cr.bb_variates(4, 5, np.arange(10)), g[5, :10])


@pytest.mark.parametrize("N", [257, 1000])
def test_se_bb_is_the_bootstrap_standard_error(N):
    """Var(sum_i alpha_i e_i) = var_pop(e) / (N + 1) under Dirichlet(1, ..., 1): se_bb^2 -> N^2 / (N + 1) var_pop(e).  A standard
    deviation estimated from B replicates has relative standard error 1 / sqrt(2 B): five of them at B = 1000 are 0.112."""
    B = 1000
    for kind in ("close", "dominant", "deep"):
        e = cr.make(N, 4, 77 + N, kind)
        w, se_bb, z, _ = cr.bb(e, B, seed=11)
        ratio = se_bb / np.sqrt(N * N / (N + 1.0) * np.var(e, axis=0))
        print("N", N, kind, "se_bb / theory", ratio)
        assert np.all(np.abs(ratio - 1.0) <= 5.0 / math.sqrt(2 * B))
        assert abs(w.sum() - 1.0) <= 1e-12 and np.all(w >= 0.0)


# ---- the header ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(INC, "compare.h")), "pymc_amd/csrc/compare.h is missing"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    out = str(tmp_path_factory.mktemp("compare") / "compare_check")
    base = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + INC, SRC, "-o", out]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return out


def _run(exe, req):
    r = subprocess.run([exe], input=req, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [[float.fromhex(t) if "x" in t else float(t) for t in ln.split()] for ln in r.stdout.splitlines()]


def _mat(e):
    return " ".join(float(v).hex() for v in e.ravel())


def test_the_headers_variates_equal_the_restatements_bit_for_bit(exe):
    cases = [(0, 0, 9, 0, 130), (12345678901234567890, 998, 4, 4990000, 70), (7, 65530, 6, (1 << 32) - 3, 6), (2 ** 63 + 5, 0, 2, (1 << 40), 3)]
    got = _run(exe, "".join(f"G {s} {b0} {nb} {i0} {ni}\n" for s, b0, nb, i0, ni in cases))
    at = 0
    for s, b0, nb, i0, ni in cases:
        ref = cr.bb_variates(s, np.arange(b0, b0 + nb, dtype=np.uint64)[:, None], np.arange(i0, i0 + ni, dtype=np.uint64)[None, :], libm=True)
        rows = np.array(got[at:at + nb])
        at += nb
        assert rows.shape == ref.shape and np.array_equal(rows, ref), (s, b0, i0)


def test_the_headers_terms_and_pass_agree_with_the_restatement(exe, solved):
    worst = 0.0
    for (N, K, kind), (e, w, f, gap, passes) in solved.items():
        if N not in (1, 65, 1000):
            continue
        got = _run(exe, f"T {N} {K} {_mat(e)}\n")
        m, p = cr.terms(e)
        rows = np.array(got)
        assert np.array_equal(rows[:, 0], m)
        np.testing.assert_allclose(rows[:, 1:], p, rtol=1e-12, atol=0.0)
        wt = np.random.default_rng(N + K).dirichlet(np.ones(K))
        out = np.array(_run(exe, f"P {N} {K} {' '.join(float(v).hex() for v in wt)} {_mat(e)}\n")[0])
        ld, g, H = cr.stack_pass(p, wt)
        ref = np.concatenate([[m.sum(), ld], g, H.ravel()])
        err = np.abs(out - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(err.max()))
        assert err.max() <= 1e-12, (N, K, kind, err.max())
    print("header pass: worst relative difference", worst)


def test_the_headers_solver_agrees_with_the_restatement(exe, solved):
    worst_f = worst_w = 0.0
    most = 0
    for (N, K, kind), (e, w, f, gap, passes) in solved.items():
        out = _run(exe, f"S {N} {K} {float(1e-12).hex()} 64 {_mat(e)}\n")[0]          # (the restatement's own tolerance)
        wh, fh, gh, ph = np.array(out[:K]), out[K], out[K + 1], int(out[K + 2])
        assert gh <= 1e-10 and ph <= 64 and np.all(wh >= 0.0) and abs(wh.sum() - 1.0) <= 1e-12, (N, K, kind, gh, ph)
        assert abs(gh - cr.kkt_gap(e, wh)) <= 1e-12
        most = max(most, ph)
        worst_f = max(worst_f, abs(fh - f) / max(1.0, abs(f)))
        assert abs(fh - f) <= 1e-12 * max(1.0, abs(f)), (N, K, kind, fh, f)
        if kind != "dup" and N >= K - 1 and cr.curvature(e, w) > 1e-6:
            worst_w = max(worst_w, float(np.abs(wh - w).max()))
            assert np.abs(wh - w).max() <= 1e-12, (N, K, kind)          # (where the maximiser is unique)
    print("header solver: worst relative objective difference", worst_f, "worst weight difference", worst_w, "most passes", most)
    assert most <= 18


def test_the_solver_stops_at_its_cap_and_reports_the_gap_it_reached(exe, solved):
    """The cap is reached without a hard input by lowering it: the header's solver returns after exactly `max_passes` passes with the
    gap of the point it stands at (one pass: the start 1 / K), and more passes never leave it with a lower objective."""
    e, w, f, gap, passes = solved[(1000, 4, "close")]
    assert passes > 2
    last = -math.inf
    for cap in (1, 2, passes):
        out = _run(exe, f"S 1000 4 {float(1e-12).hex()} {cap} {_mat(e)}\n")[0]
        wh, fh, gh, ph = np.array(out[:4]), out[4], out[5], int(out[6])
        assert ph == cap and abs(wh.sum() - 1.0) <= 1e-12 and np.all(wh >= 0.0)
        assert abs(gh - cr.kkt_gap(e, wh)) <= 1e-12 and abs(fh - cr.objective(e, wh)) <= 1e-12 * abs(fh)
        if cap == 1:
            assert np.array_equal(wh, np.full(4, 0.25))
        if cap < passes:
            assert gh > 1e-10
        else:
            assert gh <= 1e-12
        assert fh >= last
        last = fh


def test_the_program_refuses_malformed_input(exe):
    assert subprocess.run([exe], input="X 1 2\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="T 3 9 0 0 0\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="S 2 2 1e-10 64 0x1p0 -1\n", capture_output=True, text=True).returncode == 2


# ---- the public interface, host side ----------------------------------------------------------------------------------------------------
def test_compare_pointwise_refuses_bad_arguments_before_touching_the_device():
    from pymc_amd import compare as cmp

    a = np.zeros(5)
    with pytest.raises(ValueError, match="at least 2"):
        cmp.compare_pointwise({"a": a})
    with pytest.raises(ValueError, match="at most 8"):
        cmp.compare_pointwise({str(k): a for k in range(9)})
    with pytest.raises(ValueError, match="same number of observations"):
        cmp.compare_pointwise({"a": a, "b": np.zeros(6)})
    with pytest.raises(ValueError, match="method"):
        cmp.compare_pointwise({"a": a, "b": a}, method="bma")
    with pytest.raises(ValueError, match="b_samples"):
        cmp.compare_pointwise({"a": a, "b": a}, method="BB-pseudo-BMA", b_samples=0)
    with pytest.raises(ValueError, match="ic"):
        cmp.compare_pointwise({"a": a, "b": a}, ic="dic")


def test_a_solve_that_hit_its_cap_is_warned_about(monkeypatch):
    from pymc_amd import compare as cmp

    assert cmp.cap_warning(1e-10, 64, 1000) is None and cmp.cap_warning(3e-7, 63, 1000) is None and cmp.cap_warning(0.0, 64, 1000) is None
    text = cmp.cap_warning(3e-7, 64, 1000)
    assert "cap of 64 passes" in text and "kkt_gap = 3e-07" in text and "N kkt_gap = 0.0003" in text

    class Stub:
        """stands in for the device handle: a solve that stopped at `passes` with `gap`"""
        gap, passes = 3e-7, 64

        def __init__(self, N, K, device=None):
            self.K = K

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

        def set(self, k, row, order=None):
            pass

        def moments(self):
            return -np.arange(self.K, dtype="float64"), np.ones(self.K), np.ones(self.K), 0

        def stacking(self):
            return np.full(self.K, 1.0 / self.K), -1.0, self.gap, self.passes

    monkeypatch.setattr(cmp, "Comparison", Stub)
    rows = {"a": np.zeros(5), "b": np.zeros(5)}
    with pytest.warns(UserWarning, match="cap of 64 passes with kkt_gap = 3e-07"):
        out = cmp.compare_pointwise(rows)
    assert out["passes"] == 64 and out["kkt_gap"] == 3e-7 and out["names"] == ["a", "b"]
    Stub.gap, Stub.passes = 5e-11, 9
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert cmp.compare_pointwise(rows)["passes"] == 9


def test_the_calls_refuse_a_null_handle():
    import ctypes as C

    import __graft_entry__ as g

    g.build_engine()
    from pymc_amd import _lib

    lib = _lib.load()
    out = np.full(8, 7.0)
    n = C.c_int32(-1)
    assert not lib.nuts_compare_create(0, 2) and "N >= 1" in _lib.last_error()
    assert not lib.nuts_compare_create(10, 1) and not lib.nuts_compare_create(10, 9)
    assert lib.nuts_compare_set(None, 0, _lib.dptr(out), None) == _lib.NUTS_E_ARG
    assert lib.nuts_compare_moments(None, _lib.dptr(out), None, None, C.byref(n)) == _lib.NUTS_E_ARG and n.value == -1
    assert lib.nuts_compare_stacking(None, _lib.dptr(out), None, None, C.byref(n)) == _lib.NUTS_E_ARG
    assert lib.nuts_compare_bb(None, 10, 0, _lib.dptr(out), None, None) == _lib.NUTS_E_ARG
    lib.nuts_compare_destroy(None)
    assert np.all(out == 7.0)
