"""Prior draws on the host: the plan (`predictive.prior_plan`), the refusals (`predictive.prior_refusal`), the NumPy restatement of
the draws (tests/prior_reference.py) held to `scipy.stats`, and pymc_amd/csrc/prior.h -- the header k_prior_level compiles -- held
to the restatement through `tests/prior_check.cpp`, a stand-alone program (system compiler, -Wall -Wextra -Werror, address and
undefined-behaviour sanitizers when they link; it is never loaded into Python).

Bars.  Conditional uniformity: with u = F(x | the parents' drawn values), sup |ECDF(u) - u| <= 1.95 / sqrt(n), the asymptotic 0.001
level of the Kolmogorov statistic (the bar of tests/test_predictive_host.py), n = 20 000 pooled over 80 draws x 250 elements for the
vector variables; the seed is the case's number, fixed in advance.  Child against parent: |Pearson r| of the two conditional values
at the same (s, i) <= 3.29 / sqrt(n), the two-sided 0.001 level of r sqrt(n) under independence.  Header against restatement:
rtol = atol = 1e-10 on every element whose acceptance margin in the restatement exceeds 1e-9 -- the cases are chosen so that the
restatement leaves out none, which is asserted.
"""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predictive_reference as ref  # noqa: E402
import prior_models as pm_  # noqa: E402
import prior_reference as pref  # noqa: E402
from pymc_amd import model_spec as ms  # noqa: E402
from pymc_amd import models, predictive, trace  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "prior_check.cpp")
INC = os.path.join(ROOT, "pymc_amd", "csrc")
S, SIZE = 80, 250
TOL = dict(rtol=1e-10, atol=1e-10)


# ---- 1. the plan ---------------------------------------------------------------------------------------------------------------------
def test_plan_of_eight_schools_is_one_level_of_three_variables():
    assert predictive.prior_plan(models.eight_schools()) == [[("eta", 0), ("mu", 1), ("tau", 2)]]


def test_plan_of_the_extra_variant_puts_tau_before_alpha_and_everything_else_first():
    spec = models.hier_logit_variant("extra", G=4, rows_per_group=5)
    plan = predictive.prior_plan(spec)
    assert [[n for n, _ in lv] for lv in plan] == [["tau", "mu", "theta", "sigma", "z", "nu"], ["alpha"]]
    for lv in plan:
        for name, fi in lv:
            assert spec.factors[fi].name == name


def test_plan_of_a_three_deep_chain_through_a_program():
    spec = pm_.chain3()
    assert len(spec.factors[2].prog) > 0
    assert predictive.prior_plan(spec) == [[("s", 0)], [("m", 1)], [("x", 2)]]


def test_plan_of_a_child_whose_mean_gathers_a_parent():
    spec = pm_.gathered()
    assert any(o.kind == ms.OP_GATHER for o in predictive._operands(spec.factors[1], 1))
    assert predictive.prior_plan(spec) == [[("a", 0)], [("b", 1)]]


def test_plan_gives_the_mixture_nodes_weights_level_zero_and_no_factor():
    plan = predictive.prior_plan(pm_.dirichlet_mixture(K=3))
    assert plan == [[("w", -1), ("mu", 0), ("sigma", 1)]]


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(pm_.REFUSALS)), ids=[c[0] for c in pm_.REFUSALS])
def test_a_prior_out_of_scope_is_refused_by_name(case):
    _, build, text, _ = pm_.REFUSALS[case]
    spec = build()
    why = predictive.prior_refusal(spec)
    assert why is not None and text in why, why
    with pytest.raises(ValueError, match="prior predictive refused"):
        predictive.prior_plan(spec)
    with pytest.raises(ValueError, match="prior predictive refused"):
        predictive.sample_prior_predictive(spec, 3)      # (refused before a device is asked for)


def test_models_in_scope_are_not_refused():
    for spec in (models.eight_schools(), pm_.chain3(), pm_.gathered(), pm_.every_family(8), pm_.dirichlet_mixture(9), pm_.nan_model(),
                 models.hier_logit(G=6, D=3, rows_per_group=7), models.glm_nuts(N=30, P=5)):
        assert predictive.prior_refusal(spec) is None


# ---- 3. the restatement draws from the conditional distributions -----------------------------------------------------------------------
UNIFORMITY = [("every family", lambda: pm_.every_family(SIZE)), ("three deep", lambda: pm_.chain3(SIZE)),
              ("gather", lambda: pm_.gathered(N=SIZE, A=7)), ("sized", lambda: pm_.sized(SIZE))]


@pytest.fixture(scope="module")
def drawn():
    """case number -> (spec, q, margin, u): drawn once, shared, left unchanged"""
    out = {}
    for case, (_, build) in enumerate(UNIFORMITY):
        spec = build()
        q, margin = pref.sample(spec, S, seed=case)
        out[case] = (spec, q, margin, pm_.conditional_u(spec, q))
    return out


@pytest.mark.parametrize("case", range(len(UNIFORMITY)), ids=[c[0] for c in UNIFORMITY])
def test_every_variable_is_uniform_under_its_conditional_cdf(drawn, case):
    spec, q, _, u = drawn[case]
    assert np.all(np.isfinite(q))
    assert set(u) == {v.name for v in spec.vars}
    for name, uu in u.items():
        n = uu.size
        d = pm_.sup_uniform(uu)
        print(UNIFORMITY[case][0], name, "n =", n, "sup |ECDF - u| sqrt(n) =", d * math.sqrt(n))
        assert d <= 1.95 / math.sqrt(n), name


def test_the_models_cover_every_continuous_family_and_every_transform():
    spec = pm_.every_family(4)
    plan = predictive.prior_plan(spec)
    families = {spec.factors[fi].dist for lv in plan for _, fi in lv}
    assert families == {d for d in range(ms.D_DERIVED + 1) if d not in predictive.REFUSED_FAMILIES + predictive.PRIOR_DISCRETE}
    assert {v.transform for v in spec.vars} == {ms.TR_NONE, ms.TR_LOG, ms.TR_LOGODDS, ms.TR_INTERVAL}
    un = next(v for v in spec.vars if v.name == "un")
    assert (un.lower, un.upper) == (-1.0, 3.0)


@pytest.mark.parametrize("case", range(len(UNIFORMITY)), ids=[c[0] for c in UNIFORMITY])
def test_a_child_does_not_reuse_its_parents_block(drawn, case):
    spec, _, _, u = drawn[case]
    pairs = pm_.parents_elementwise(spec)
    assert pairs or UNIFORMITY[case][0] == "gather"
    for child, parent in pairs:
        a, b = np.ravel(u[child]), np.ravel(u[parent])
        r = float(np.corrcoef(a, b)[0, 1])
        print(UNIFORMITY[case][0], child, "|", parent, "n =", a.size, "r sqrt(n) =", r * math.sqrt(a.size))
        assert abs(r) <= 3.29 / math.sqrt(a.size), (child, parent)


def test_transforms_round_trip_through_the_traces_backward():
    spec = pm_.every_family(16)
    q, _ = pref.sample(spec, 5, seed=1)
    x = pref.constrained(spec, q)
    for v in spec.vars:
        blk = x[:, v.offset : v.offset + v.size]
        np.testing.assert_allclose(trace.backward(v, pref.forward(v, blk)), blk, rtol=1e-12, atol=1e-12)


def test_deterministics_of_the_prior_are_the_trace_backends():
    """`prior` holds the Deterministics by the evaluation the trace backend records them with: same values, same shapes (a
    one-element Deterministic is a scalar per draw)"""
    from pymc_amd import backends

    spec = pm_.with_deterministics()
    q, _ = pref.sample(spec, 7, seed=4)
    got = predictive.constrained_from_positions(spec, q[None])
    tr = backends.NDArray(model=spec)
    tr.setup(7, 0)
    tr.record_batch(q, None)
    assert list(got) == ["s", "x", "s2", "ex"] and got["s2"].shape == (1, 7) and got["ex"].shape == (1, 7, 6)
    for name in got:
        assert np.array_equal(got[name][0], tr.samples[name]), name
    np.testing.assert_allclose(got["s2"], got["s"] ** 2, rtol=1e-14)
    np.testing.assert_allclose(got["ex"], np.exp(got["x"]) * got["s"][..., None], rtol=1e-14)


# ---- 4. the Dirichlet draw -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 9])
def test_the_dirichlet_draw_has_beta_marginals_and_inverts(K):
    n = 20000
    alpha = np.linspace(0.6, 2.4, K)
    y, w, _ = pref.dirichlet(alpha, seed=K, index=2, s=np.arange(n))
    assert y.shape == (n, K - 1) and np.all(np.isfinite(y))
    for k in range(K):
        d = pm_.sup_uniform(stats.beta.cdf(w[:, k], alpha[k], alpha.sum() - alpha[k]))
        print("Dirichlet K", K, "w", k, "sup |ECDF - u| sqrt(n) =", d * math.sqrt(n))
        assert d <= 1.95 / math.sqrt(n)
    var = ms.FreeVar("w", (K - 1,), simplex=True)
    np.testing.assert_allclose(trace.backward(var, y), w, rtol=0, atol=1e-12)


def test_prior_streams_differ_from_those_of_observed_nodes_and_from_each_other():
    i = np.arange(1000)
    base = pref.Address(1, 0, 0, i).block(0)[0]
    for kind in range(4):
        assert not np.any(ref.Address(1, kind, 0, 0, i).block(0)[0] == base)
    for other in (pref.Address(2, 0, 0, i), pref.Address(1, 1, 0, i), pref.Address(1, 0, 1, i)):
        assert not np.any(other.block(0)[0] == base)


# ---- 5. the header -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(INC, "prior.h")), "pymc_amd/csrc/prior.h is missing"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    out = str(tmp_path_factory.mktemp("prior") / "prior_check")
    base = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + INC, SRC, "-o", out]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return out


def _floats(text):
    return np.array([float("nan") if w in ("nan", "-nan") else float.fromhex(w) if "x" in w else float(w) for w in text.split()])


def _run(exe, req, code=0):
    r = subprocess.run([exe], input=req, capture_output=True, text=True)
    assert r.returncode == code, (r.returncode, r.stderr)
    return r.stdout


def _tok(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("inf" if v == math.inf else ("-inf" if v == -math.inf else v.hex()))


# (label, dist, a1, a2, a3, transform, lower, upper)
HEADER_CASES = [
    ("normal none", ref.D_NORMAL, 1.5, 2.0, 0.0, ms.TR_NONE, 0.0, 1.0),
    ("halfnormal log", ref.D_HALFNORMAL, 1.3, 0.0, 0.0, ms.TR_LOG, 0.0, 1.0),
    ("lognormal log", ref.D_LOGNORMAL, 0.2, 0.7, 0.0, ms.TR_LOG, 0.0, 1.0),
    ("cauchy none", ref.D_CAUCHY, -1.0, 2.0, 0.0, ms.TR_NONE, 0.0, 1.0),
    ("halfcauchy log", ref.D_HALFCAUCHY, 1.5, 0.0, 0.0, ms.TR_LOG, 0.0, 1.0),
    ("laplace none", ref.D_LAPLACE, 0.5, 1.2, 0.0, ms.TR_NONE, 0.0, 1.0),
    ("exponential log", ref.D_EXPONENTIAL, 2.5, 0.0, 0.0, ms.TR_LOG, 0.0, 1.0),
    ("uniform interval", ref.D_UNIFORM, -1.0, 3.0, 0.0, ms.TR_INTERVAL, -1.0, 3.0),
    ("gamma 0.5 log", ref.D_GAMMA, 0.5, 2.0, 0.0, ms.TR_LOG, 0.0, 1.0),
    ("gamma 2.5 log", ref.D_GAMMA, 2.5, 2.0, 0.0, ms.TR_LOG, 0.0, 1.0),
    ("invgamma log", ref.D_INVGAMMA, 3.0, 2.0, 0.0, ms.TR_LOG, 0.0, 1.0),
    ("beta logodds", ref.D_BETA, 0.7, 2.5, 0.0, ms.TR_LOGODDS, 0.0, 1.0),
    ("studentt none", ref.D_STUDENTT, 4.0, 1.0, 2.0, ms.TR_NONE, 0.0, 1.0),
]
HN, HS, HI = 2000, 3, 7      # elements, draws, variable index of the header cases


def _hold(label, got, want, margin):
    """rtol = atol = 1e-10 on the elements whose acceptance margin exceeds 1e-9; at most 1 in 1 000 left out -> (max error, left out)"""
    assert got.shape == want.shape, label
    keep = margin > 1e-9
    left_out = int((~keep).sum())
    err = float(np.max(np.abs(got[keep] - want[keep]) / np.maximum(1.0, np.abs(want[keep])))) if keep.any() else 0.0
    print(label, "left out (acceptance margin <= 1e-9):", left_out, "of", got.size, "; max relative error", err)
    assert left_out * 1000 <= got.size, label
    np.testing.assert_allclose(got[keep], want[keep], err_msg=label, **TOL)
    return err, left_out


@pytest.mark.parametrize("case", range(len(HEADER_CASES)), ids=[c[0] for c in HEADER_CASES])
def test_the_header_reproduces_the_restatement(exe, case):
    label, dist, a1, a2, a3, tr, lo, hi = HEADER_CASES[case]
    req = f"draw {dist} {_tok(a1)} {_tok(a2)} {_tok(a3)} {tr} {_tok(lo)} {_tok(hi)} {case} {HI} 5 {HS} 0 {HN}\n"
    got = _floats(_run(exe, req)).reshape(HS, HN)
    val, margin = pref.draw(dist, a1, a2, a3, pref.Address(case, HI, (5 + np.arange(HS))[:, None], np.arange(HN)[None, :]))
    want = pref.forward(ms.FreeVar("v", (HN,), tr, lo, hi), val)
    assert np.all(np.isfinite(want)) and not np.any(margin <= 1e-9), "the case leaves out elements in the restatement alone"
    _hold(label, got, want, margin)


@pytest.mark.parametrize("K", [3, 9])
def test_the_header_reproduces_the_dirichlet_draw(exe, K):
    alpha = np.linspace(0.6, 2.4, K)
    ns = 500
    got = _floats(_run(exe, f"dirichlet {K} " + " ".join(_tok(a) for a in alpha) + f" {K} 4 0 {ns}\n")).reshape(ns, K - 1)
    want, _, margin = pref.dirichlet(alpha, seed=K, index=4, s=np.arange(ns))
    assert not np.any(margin <= 1e-9), "the case leaves out draws in the restatement alone"
    _hold(f"dirichlet K={K}", got, want, np.broadcast_to(margin[:, None], want.shape))


def test_the_forward_transforms_keep_infinities_and_nan(exe):
    """at 0, 1, the bounds, the smallest and largest doubles inside the bounds, and NaN: +-inf or NaN where the mathematics says so,
    finite just inside; nothing traps (the program runs under the sanitizers where they link) and nothing is clamped"""
    lo, hi = -1.0, 3.0
    inside = [np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0), np.nextafter(lo, hi), np.nextafter(hi, lo)]
    xs = [0.0, 1.0, lo, hi, math.nan, -0.5, math.inf] + inside
    req = "".join(f"forward {tr} {_tok(lo)} {_tok(hi)} {_tok(x)}\n" for tr in (ms.TR_LOG, ms.TR_LOGODDS, ms.TR_INTERVAL, ms.TR_NONE) for x in xs)
    got = _floats(_run(exe, req)).reshape(4, len(xs))
    want = np.array([pref.forward(ms.FreeVar("v", (), tr, lo, hi), np.array(xs)) for tr in (ms.TR_LOG, ms.TR_LOGODDS, ms.TR_INTERVAL, ms.TR_NONE)])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(np.sign(got[np.isinf(got)]), np.sign(want[np.isinf(want)]))
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], **TOL)
    log_, odds, itv = got[0], got[1], got[2]
    assert log_[0] == -math.inf and math.isnan(log_[5]) and log_[6] == math.inf and np.isfinite(log_[7])
    assert odds[0] == -math.inf and odds[1] == math.inf and math.isnan(odds[4]) and math.isnan(odds[5]) and np.all(np.isfinite(odds[7:9]))
    assert itv[2] == -math.inf and itv[3] == math.inf and math.isnan(itv[4]) and np.all(np.isfinite(itv[9:11]))
    assert np.array_equal(got[3][:4], np.array(xs[:4])) and math.isnan(got[3][4])


def test_the_64_counters_of_a_prior_variate_differ_from_those_of_every_observed_node(exe):
    """equal (seed, s, i, index), kinds 0 .. 3, blocks t = 0 .. 63: the program prints both counters' words; the second word of the
    prior's has bit 31 set and the node's has not, whatever the other three are"""
    out = _run(exe, "counters 5 77 123456789012 63\n").split()
    words = np.array([int(w, 16) for w in out], dtype=np.uint64).reshape(64, 5, 4)      # [t][prior, kind 0 .. 3][word]
    prior, nodes = words[:, 0], words[:, 1:]
    assert np.all(prior[:, 1] & np.uint64(0x80000000)) and not np.any(nodes[:, :, 1] & np.uint64(0x80000000))
    for k in range(4):
        assert np.all(np.any(prior != nodes[:, k], axis=1))
    assert np.array_equal(prior[:, 3], np.uint64(5 << 16) | np.arange(64, dtype=np.uint64))
    assert np.array_equal(nodes[:, 2, 3], np.uint64(2 << 30 | 5 << 16) | np.arange(64, dtype=np.uint64))


def test_the_header_refuses_an_index_beyond_14_bits(exe):
    _run(exe, "draw 0 0 1 0 0 0 1 1 16384 0 1 0 1\n", code=4)
    _run(exe, "draw 11 0 1 0 0 0 1 1 0 0 1 0 1\n", code=4)       # TruncatedNormal
    _run(exe, "draw 17 1 0 0 0 0 1 1 0 0 1 0 1\n", code=4)       # Poisson: a prior is continuous
