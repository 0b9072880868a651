"""The convergence summary on the host: the NumPy restatement (tests/summary_reference.py) is the estimators of pymc_amd/stats.py
and of the closed forms, and pymc_amd/csrc/summary.h -- the header k_summary compiles -- reproduces it.

`tests/summary_check.cpp` is a stand-alone program around the header (system compiler, -Wall -Wextra -Werror, address and
undefined-behaviour sanitizers when they link); it is never loaded into Python.
"""
import math
import os
import shutil
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scalar_edges as se  # noqa: E402
import summary_reference as sr  # noqa: E402

from pymc_amd import stats  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "summary_check.cpp")
INC = os.path.join(ROOT, "pymc_amd", "csrc")
KAT = os.path.join(ROOT, "tests", "golden", "stats_kat.npz")
KAT_NAMES = ("iid", "ar1", "anti", "shifted", "drift", "ties")
SHAPES = [(1, 8), (2, 9), (3, 101), (4, 100), (1, 7), (2, 400)]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KAT_NAMES)
def test_the_restatement_reproduces_the_known_answers(name):
    k = np.load(KAT)
    out = sr.summarize_one(k[name + "_x"])
    np.testing.assert_allclose(out["ess_bulk"], float(k[name + "_ess_bulk"]), rtol=1e-10)
    np.testing.assert_allclose(out["r_hat"], float(k[name + "_rhat"]), rtol=1e-10)


def test_the_restatement_is_stats_py():
    worst_e = worst_r = 0.0
    for C, N in SHAPES:
        for label, x in sr.kinds(C, N, 100 * C + N):
            if not np.all(np.isfinite(x)):
                assert all(math.isnan(v) for v in sr.summarize_one(x).values()), label
                continue
            out = sr.summarize_one(x)
            with np.errstate(all="ignore"):
                e, r = stats.ess_bulk(x), stats.rhat(x)
            for got, ref in ((out["ess_bulk"], e), (out["r_hat"], r)):
                assert (math.isnan(got) and math.isnan(ref)) or abs(got - ref) <= 1e-10 * abs(ref), (C, N, label, got, ref)
            if math.isfinite(e):
                worst_e, worst_r = max(worst_e, abs(out["ess_bulk"] - e) / e), max(worst_r, abs(out["r_hat"] - r))
            # the direct and the FFT autocovariance end the scan at the same lag for every array an ESS is taken of
            s = sr.split(x)
            d = (x - x.mean()) ** 2
            for a in (s, sr.split(d), sr.split((x <= np.quantile(x, 0.05)).astype("float64"))):
                ref = stats._ess_raw(a)
                got = sr.ess(a)
                assert (math.isnan(got) and math.isnan(ref)) or abs(got - ref) <= 1e-10 * abs(ref), (C, N, label, got, ref)
    print("restatement vs stats.py: worst relative ess_bulk", worst_e, "worst r_hat", worst_r)


def test_small_shapes_and_non_finite_draws():
    x = np.random.default_rng(2).standard_normal((1, 7))
    out = sr.summarize_one(x)                     # N // 2 = 3 < 4: no ESS, hence no MCSE
    assert all(math.isnan(out[k]) for k in ("ess_bulk", "ess_tail", "mcse_mean", "mcse_sd"))
    assert all(math.isfinite(out[k]) for k in ("mean", "sd", "hdi_lo", "hdi_hi", "r_hat"))
    out = sr.summarize_one(x[:, :1])              # one draw: nothing to split
    assert out["mean"] == x[0, 0] and all(math.isnan(out[k]) for k in sr.COLUMNS if k not in ("mean", "hdi_lo", "hdi_hi"))
    assert sr.hdi_sorted(np.arange(5.0), 0.9999) == (0.0, 4.0) and sr.hdi_sorted(np.arange(5.0), 0.1) == (0.0, 0.0)
    assert all(math.isnan(v) for v in sr.hdi_sorted(np.arange(5.0), 1.0))      # S - k < 1


def test_quantile_is_numpy_quantile():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 8, 21, 400, 8000):
        for xs in (np.sort(rng.standard_normal(n)), np.sort(np.round(2.0 * rng.standard_normal(n)) / 2.0)):
            for q in (0.05, 0.95, 0.5, 0.0, 1.0, 0.25):
                assert sr.quantile_sorted(xs, q) == float(np.quantile(xs, q)), (n, q)


def test_closed_forms():
    """iid draws: every ESS ~ S within the band tests/test_stats.py holds the bulk-ESS to (12 %), so mcse_mean ~ sd / sqrt(S) within
    the square root of that band; the HDI of 0 .. S-1 is (0, k) exactly (every window has width k: the first wins)."""
    x = np.random.default_rng(11).normal(size=(4, 1000, 4))
    S = 4000
    out = sr.summarize(x)
    ess_mean = (out["sd"] / out["mcse_mean"]) ** 2
    print("iid: ess_tail / S", out["ess_tail"] / S, "ess behind mcse_mean / S", ess_mean / S)
    assert np.all(np.abs(out["ess_tail"] / S - 1.0) < 0.12) and np.all(np.abs(ess_mean / S - 1.0) < 0.12)
    ratio = out["mcse_mean"] / (out["sd"] / math.sqrt(S))
    assert np.all((ratio > 1.0 / math.sqrt(1.12)) & (ratio < 1.0 / math.sqrt(0.88)))
    # Var(sd) ~ sd^2 / (2 S) for normal draws
    assert np.all(np.abs(out["mcse_sd"] / (out["sd"] / math.sqrt(2 * S)) - 1.0) < 0.12)
    for S, prob in ((100, 0.94), (101, 0.5), (8, 0.94)):
        k = int(math.floor(prob * S))
        perm = np.random.default_rng(S).permutation(S).astype("float64")
        o = sr.summarize_one(perm[None, :], prob)
        assert (o["hdi_lo"], o["hdi_hi"]) == (0.0, float(k))


# ---- the header ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(INC, "summary.h")), "pymc_amd/csrc/summary.h is missing"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    out = str(tmp_path_factory.mktemp("summary") / "summary_check")
    base = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + INC, SRC, "-o", out]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return out


def _tok(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("inf" if v == math.inf else ("-inf" if v == -math.inf else v.hex()))


def _run(exe, requests):
    """requests: lists of numbers -> the flat list of results"""
    req = "".join(" ".join(_tok(v) for v in r) + "\n" for r in requests)
    r = subprocess.run([exe], input=req, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return [float("nan") if w in ("nan", "-nan") else float.fromhex(w) if "x" in w else float(w) for w in r.stdout.split()]


def _same(got, ref, tol):
    return (math.isnan(got) and math.isnan(ref)) or abs(got - ref) <= tol * abs(ref)


def _arrays():
    """(label, (chains, draws)) in split layout: what the five scans of a parameter see"""
    out = []
    for C, N in SHAPES:
        for label, x in sr.kinds(C, N, 7 * C + N):
            if not np.all(np.isfinite(x)):
                continue
            s = sr.split(x)
            d = (x - x.mean()) ** 2
            tag = f"{C}x{N} {label}"
            out += [(tag + " x", s), (tag + " z", sr.z_scale(s)), (tag + " d", sr.split(d)),
                    (tag + " I05", sr.split((x <= sr.quantile_sorted(np.sort(x.ravel()), 0.05)).astype("float64"))),
                    (tag + " folded z", sr.z_scale(np.abs(s - np.median(s))))]
    k = np.load(KAT)
    out += [("kat " + n, sr.z_scale(sr.split(k[n + "_x"]))) for n in KAT_NAMES]
    out.append(("one chain", np.random.default_rng(5).standard_normal((1, 50))))
    return out


def test_the_header_reproduces_the_geyer_scan_and_rhat(exe):
    arrays = _arrays()
    ess = _run(exe, [[1, a.shape[0], a.shape[1], *a.ravel()] for _, a in arrays])
    rh = _run(exe, [[2, a.shape[0], a.shape[1], *a.ravel()] for _, a in arrays if a.shape[0] > 1])
    assert len(ess) == len(arrays)
    worst_e = worst_r = 0.0
    with np.errstate(all="ignore"):
        for (label, a), got in zip(arrays, ess):
            ref = sr.ess(a)
            assert _same(got, ref, 1e-12), (label, got, ref)
            if math.isfinite(ref):
                worst_e = max(worst_e, abs(got - ref) / ref)
        for (label, a), got in zip([t for t in arrays if t[1].shape[0] > 1], rh):
            ref = sr.rhat_of(a)
            assert _same(got, ref, 1e-12), (label, got, ref)
            if math.isfinite(ref):
                worst_r = max(worst_r, abs(got - ref) / ref)
    print("header: worst relative ESS difference", worst_e, "worst relative R-hat difference", worst_r)


def test_the_header_reproduces_hdi_and_quantile(exe):
    rng = np.random.default_rng(9)
    cases = []
    for S in (1, 2, 3, 8, 9, 100, 303, 8000):
        cases += [rng.standard_normal(S), np.round(2.0 * rng.standard_normal(S)) / 2.0, rng.standard_cauchy(S), np.full(S, 2.5),
                  rng.permutation(S).astype("float64")]
    for prob in (0.94, 0.5, 0.05, 0.9999):
        got = _run(exe, [[3, len(v), prob, *v] for v in cases])
        ref = [w for v in cases for w in sr.hdi_sorted(np.sort(v), prob)]
        assert np.array_equal(np.array(got), np.array(ref), equal_nan=True), prob
    for q in (0.05, 0.95, 0.5, 0.0, 1.0):
        got = _run(exe, [[4, len(v), q, *v] for v in cases])
        assert np.array_equal(np.array(got), np.array([sr.quantile_sorted(np.sort(v), q) for v in cases])), q
        assert np.array_equal(np.array(got), np.array([float(np.quantile(v, q)) for v in cases])), q


def _ndtri_points():
    pts = [(r - 0.375) / (S + 0.25) for S in (4, 8192) for r in (1, S // 2, S)]
    edge = math.exp(-25.0)                          # r = sqrt(-log p) = 5, the edge between the two tail branches
    pts += se.near(0.075, 0.925, edge) + se.near(1.0 - edge)[:2] + [0.5, 1e-300, 1.0 - 2.0 ** -53]
    return pts


def test_ndtri_against_mpmath(exe):
    """AS241 PPND16 in the project's error measure (tests/scalar_edges.py: error in ulps of the result plus what one ulp of the
    argument may move it), held to the project's 4 ulp-equivalents."""
    pts = _ndtri_points()
    got = _run(exe, [[5, p] for p in pts])
    worst = 0.0
    with mp.workprec(se.PREC):
        for p, a in zip(pts, got):
            t = mp.sqrt(2) * mp.erfinv(2 * mp.mpf(p) - 1)
            sens = mp.sqrt(2 * mp.pi) * mp.exp(t * t / 2)
            e = se.measure(a, t, [sens], [p])
            print(f"ndtri({p!r}) = {a!r}: {e:.3f} ulp-equivalents")
            worst = max(worst, e)
            assert e <= 4.0, (p, a, e)
    print("ndtri: worst error", worst, "ulp-equivalents")
    assert _run(exe, [[5, 0.0], [5, 1.0]]) == [-math.inf, math.inf]


def test_the_program_refuses_malformed_input(exe):
    assert subprocess.run([exe], input="1 2 3 0x1p0\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="7 1\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="5 1.0x\n", capture_output=True, text=True).returncode == 2


# ---- the Python entry points, as far as they go without a device --------------------------------------------------------------------
def test_names_are_arviz_labels():
    from pymc_amd import summary

    assert summary.flat_names("tau", ()) == ["tau"]
    assert summary.flat_names("theta", (3,)) == ["theta[0]", "theta[1]", "theta[2]"]
    assert summary.flat_names("L", (2, 2)) == ["L[0, 0]", "L[0, 1]", "L[1, 0]", "L[1, 1]"]
    assert summary.COLUMNS == sr.COLUMNS


def test_refusals_need_no_device():
    import __graft_entry__ as g

    g.build_engine()
    from pymc_amd import _lib, summary

    lib = _lib.load()
    limit = lib.nuts_summary_max_draws()
    assert limit == summary.max_draws() == 8192
    x = np.zeros((1, limit + 1, 2))
    out = np.full((9, 2), 7.0)
    assert lib.nuts_summary(_lib.dptr(x), 1, limit + 1, 2, 0.94, _lib.dptr(out)) == _lib.NUTS_E_ARG and "8192" in _lib.last_error()
    for C, N, prob in ((0, 5, 0.94), (2, 0, 0.94), (2, 5, 0.0), (2, 5, 1.0), (2, 5, float("nan"))):
        assert lib.nuts_summary(_lib.dptr(x), C, N, 2, prob, _lib.dptr(out)) == _lib.NUTS_E_ARG, (C, N, prob)
    assert np.all(out == 7.0)
    with pytest.raises(ValueError, match="8192.*out of scope"):
        summary.summarize(x)
    with pytest.raises(ValueError, match="hdi_prob"):
        summary.summarize(np.zeros((2, 8, 1)), hdi_prob=1.5)
