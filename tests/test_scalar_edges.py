"""The scalar functions of pymc_amd/csrc/scalar_math.h and the oracle's scalar ops against mpmath at the edges of their domains,
on the host (measure, regimes and point tables: tests/scalar_edges.py).

`tests/scalar_math_check.cpp` is a stand-alone program around the header (system compiler, -Wall -Wextra -Werror, address and
undefined-behaviour sanitizers when they link): what the device compiles is what runs here, with the host's libm under it.  Every
regime of the six functions must stay within 16 max(1, E_O) of the truth.  The oracle (oracle/ref_models.py `_instr_value`) is held
to the same truths: its error per regime IS the tabulated E_O (asserted from both sides, so the table cannot go stale), and the
isolating models the device test uses are checked on it bit for bit.
"""
import os
import shutil
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scalar_edges as se  # noqa: E402

from oracle import ref_models  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "scalar_math_check.cpp")
INC = os.path.join(ROOT, "pymc_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    out = str(tmp_path_factory.mktemp("scalar_math") / "scalar_math_check")
    # (-ffp-contract=off: no fused multiply-add the source does not spell out, on any host)
    base = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + INC, SRC, "-o", out]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return out


def _run(exe, fn, pts):
    req = "".join(fn + " " + " ".join(float(c).hex() for c in p) + "\n" for p in pts)
    r = subprocess.run([exe], input=req, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [float.fromhex(w) if w not in ("nan", "-nan") else float("nan") for w in r.stdout.split()]
    assert len(out) == len(pts)
    return np.asarray(out)


def test_the_program_refuses_what_it_does_not_know(exe):
    assert subprocess.run([exe], input="lgamma 0x1p0\n", capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe], input="softplus 1.0x\n", capture_output=True, text=True).returncode == 2
    assert _run(exe, "logaddexp", [(float("-inf"), float("-inf"))])[0] == float("-inf")


def test_the_gamma_family_truth_agrees_with_mpmath():
    """tests/scalar_edges.py restates log|Gamma|, psi, psi', psi'' (mpmath's polygamma takes minutes at 2000 bits): 200 bits here"""
    with mp.workprec(200):
        for x in (0.3, se.DIGAMMA_ROOT, -2.5, -1000.7, 50.0, 1e8, 1e-8, 1e-300, 171.5, -0.999999999, se.DIGAMMA_NEG_ROOT):
            got = se.gamma_family(mp.mpf(x))
            want = [mp.log(abs(mp.gamma(mp.mpf(x))))] + [mp.psi(n, mp.mpf(x)) for n in range(3)]
            for g, w in zip(got, want):
                assert abs(g - w) <= mp.ldexp(1, -150) * max(abs(w), abs(mp.psi(1, mp.mpf(x))) * mp.ldexp(1, -40)), (x, g, w)


def test_the_measure():
    one = mp.mpf(1)
    assert se.measure(1.0 + 2.0 ** -52, one, [mp.mpf(0)], (1.0,)) == 1.0              # one ulp of the result
    assert se.measure(1.0 + 2.0 ** -52, one, [one], (1.0,)) == 0.5                     # ... shared with one ulp of the input
    assert se.measure(float("nan"), one, [one], (1.0,)) == float("inf")
    assert se.measure(5e-324, mp.mpf(0), [mp.mpf(0)], (1.0,)) == 1.0                    # ulp(0) is the smallest denormal


@pytest.mark.parametrize("op", sorted(se.POINTS))
def test_the_oracle_error_per_regime_is_the_tabulated_one(op):
    got = se.reference_regime_errors(op)
    assert got, op
    assert set(got) == {k for k in se.E_O if k.startswith(op + "/")}, sorted(set(got) ^ {k for k in se.E_O if k.startswith(op + "/")})
    for k, e in got.items():
        print(f"{k}: E_O = {e:.4g} (table {se.E_O[k]:.4g})")
        assert e <= se.E_O[k] <= 1.5 * e + 1.0, (k, e, se.E_O[k])


def test_every_finite_point_is_in_an_accuracy_model_and_no_other():
    groups = se.accuracy_groups()
    assert len(groups) <= 10
    seen = {}
    for _, g in groups:
        for op, idx in g:
            seen.setdefault(op, []).extend(idx)
    for op in se.POINTS:
        acc, conv = se.split_points(op)
        assert sorted(seen.get(op, [])) == sorted(acc), op
        assert sorted(acc + conv) == list(range(len(se.POINTS[op])))
        for i in acc:
            se.regime_of(op, se.POINTS[op][i])


HEADER = [("softplus", "softplus", "v"), ("sigmoid", "sigmoid", "v"), ("log1mexp", "log1mexp", "v"), ("logaddexp", "logaddexp", "v"),
          ("digamma", "digamma", "v"), ("trigamma", "digamma", "dx"), ("digamma", "gammaln", "dx"), ("sigmoid", "softplus", "dx")]


@pytest.mark.parametrize("fn,op,output", HEADER, ids=[f"{f}-as-{o}.{w}" for f, o, w in HEADER])
def test_the_header_stays_within_its_bound_in_every_regime(exe, fn, op, output):
    """`fn` of scalar_math.h at the points of `op`, as the value or the derivative the device takes it for"""
    got = se.regime_errors(op, {output: _run(exe, fn, se.POINTS[op])})
    assert got
    for k, e in got.items():
        print(f"{fn} as {k}: E = {e:.4g}, bound {se.bound(k):.4g}")
    bad = {k: (e, se.bound(k)) for k, e in got.items() if not e <= se.bound(k)}
    assert not bad, bad


def test_the_header_at_the_convention_points(exe):
    """class for class with the oracle where the truth is not finite (softplus beyond the exponent range, log1mexp at and above 0)"""
    for fn in ("softplus", "log1mexp"):
        pts = se.CONVENTION_POINTS[fn]
        got, want = _run(exe, fn, pts), se.oracle_outputs(fn, pts)["v"]
        assert [se.klass(a) for a in got] == [se.klass(a) for a in want], (fn, got, want)


@pytest.mark.parametrize("gather", [False, True], ids=["aligned", "gathered"])
def test_the_isolating_models_return_the_ops_bit_for_bit_on_the_oracle(gather):
    for name, g in se.accuracy_groups() + [("conventions", se.convention_groups())]:
        groups = [(op, pts) for op, pts in se.group_points(g)]
        spec, q, layout = se.build_model(groups, gather=gather)
        with np.errstate(all="ignore"):
            lp, grad = ref_models.evaluate(spec, q)
        assert name == "conventions" or np.isfinite(lp), (name, lp)
        for (op, pts), where in zip(groups, layout):
            want, got = se.oracle_outputs(op, pts), se.read_outputs(where, grad)
            for o in want:
                assert np.array_equal(got[o] + 0.0, want[o] + 0.0, equal_nan=True), (name, op, o, got[o], want[o])


def test_the_oracle_error_per_density_case_is_the_tabulated_one():
    """oracle/ref_models.py `_dist` (element-wise log-density and partials w.r.t. the parameters) against mpmath"""
    got = se.reference_density_errors()
    assert set(got) == set(se.E_O_DENSITY), sorted(set(got) ^ set(se.E_O_DENSITY))
    for k, e in got.items():
        print(f"{k}: E_O = {e:.4g} (table {se.E_O_DENSITY[k]:.4g})")
        assert e <= se.E_O_DENSITY[k] <= 1.5 * e + 1.0, (k, e, se.E_O_DENSITY[k])


def test_the_density_models_isolate_their_elements_on_the_oracle():
    """the gradient of a Flat parameter vector is the factor's partial, element by element, and every log-density is finite"""
    for name, cases in se.density_models():
        spec, q, layout = se.build_density_model(cases)
        with np.errstate(all="ignore"):
            lp, grad = ref_models.evaluate(spec, q)
        assert np.isfinite(lp), (name, lp)
        for c, where, o in zip(cases, layout, se.oracle_density_outputs(spec, q, cases)):
            assert np.all(np.isfinite(o["lp"])), c["name"]
            for k, ix in enumerate(where):
                assert np.array_equal(grad[ix] + 0.0, o[f"d{k + 1}"] + 0.0), (c["name"], k)


def test_the_oracle_error_of_free_variables_and_transforms_is_the_tabulated_one():
    """oracle/ref_models.py `backward` and the densities' d0: d/dq (logp(x(q)) + log|dx/dq|) against mpmath"""
    got = se.reference_free_errors()
    assert set(got) == set(se.E_O_FREE), sorted(set(got) ^ set(se.E_O_FREE))
    for k, e in got.items():
        print(f"{k}: E_O = {e:.4g} (table {se.E_O_FREE[k]:.4g})")
        assert e <= se.E_O_FREE[k] <= 1.5 * e + 1.0, (k, e, se.E_O_FREE[k])
    acc, conv = se.free_split()
    for name, pts in se.FREE_CASES.items():
        assert sorted(acc[name] + conv[name]) == list(range(len(pts)))
