"""Model comparison on the device (csrc/compare.h, compare_kernel.h, `nuts_compare_*`, pymc_amd/compare.py) against the NumPy
restatement (tests/compare_reference.py).

Inputs: `compare_reference.grid()` -- N in {1, 2, 63, 64, 65, 257, 1000, 4097} x K in {2, 3, 4, 8} x {close, dominant, deep, dup} --
with the number of workgroups chosen from N and forced to 1 and to 3 (NUTS_COMPARE_WGS; at N = 4097 every thread then has several
observations and the last one a ragged tail).

Bars.  Moments: 1e-9 relative (a double sum of <= 4097 terms is good to N 2^-53: three decades of slack), `best` exact.  Stacking:
weights >= 0 with sum 1 to 1e-12; the returned kkt_gap equals a NumPy recomputation from the returned weights to 1e-9, is <= 1e-8 and
took <= 64 passes; objective >= reference - N 1e-8 - 1e-9 |f|; for non-`dup` inputs |w - w_ref| <= sqrt(2e-8 / lambda), the
strong-concavity bound of a gap of 1e-8 (lambda as tests/test_compare_host.py explains: where it is 0 -- N < K - 1 -- the bound is
vacuous and the objective decides, as for `dup`).  Bootstrap: z within 1e-9 N sum_i g |e_ik| / sum_i g of the restatement, weights
within 1e-9 (absolute: they lie in [0, 1]) and se_bb within 1e-9 relative -- except at N = 1, where se_bb is 0 in exact arithmetic
and both sides are asserted to be 0 to 1e-9 |e|; a replicate does not depend on b_samples, bit for bit.

Measured on an MI355X (profiles/compare.json): moments 7.2e-15; kkt_gap <= 8.6e-11 after <= 10 passes, gap against NumPy 1.8e-14,
objective short of the reference by <= 1.2e-13 N, weights within 3.5e-10; z 1.1e-15 of its scale, BB weights 1.1e-13, se_bb 4.4e-11.

With PYMC_AMD_COMPARE_JSON set to a path, the run writes the measured maxima there (profiles/compare.json).
"""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compare_reference as cr  # noqa: E402
from test_gpu_loglik import rows_model  # noqa: E402

from pymc_amd import compare as cmp  # noqa: E402
from pymc_amd import loglik  # noqa: E402
from pymc_amd.model_spec import ModelBuilder  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED = {}
WGS = [None, 1, 3]


def _note(key, **vals):
    slot = MEASURED.setdefault(key, {})
    for k, v in vals.items():
        slot[k] = max(slot.get(k, 0.0), float(v))


@pytest.fixture(scope="module")
def ref():
    """(N, K, kind) -> the input and everything the restatement says about it, computed once and left unchanged"""
    made = {}

    def get(N, K, kind):
        key = (N, K, kind)
        if key not in made:
            seed = next(s for n, k, kd, s in cr.grid() if (n, k, kd) == key)
            e = cr.make(N, K, seed, kind)
            e.setflags(write=False)
            w, f, gap, passes = cr.solve(e)
            made[key] = {"e": e, "moments": cr.moments(e), "w": w, "f": f, "lam": None if kind == "dup" else cr.curvature(e, w), "bb": {}}
        return made[key]

    yield get
    path = os.environ.get("PYMC_AMD_COMPARE_JSON")
    if path and MEASURED:
        with open(path, "w") as fh:
            json.dump(MEASURED, fh, indent=1, sort_keys=True)


def _handle(e, order=None):
    N, K = e.shape
    c = cmp.Comparison(N, K, device=0)
    for k in range(K):
        c.set(k, e[:, k] if order is None else e[order, k], order)
    return c


def _wgs(monkeypatch, wgs):
    monkeypatch.setenv("PYMC_AMD_HONOUR_NUTS_ENV", "1")
    if wgs is None:
        monkeypatch.delenv("NUTS_COMPARE_WGS", raising=False)
    else:
        monkeypatch.setenv("NUTS_COMPARE_WGS", str(wgs))


@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("N", cr.N_LIST)
def test_moments_and_stacking_on_the_grid(N, wgs, ref, monkeypatch):
    _wgs(monkeypatch, wgs)
    for K in cr.K_LIST:
        for kind in cr.KINDS:
            r = ref(N, K, kind)
            e = r["e"]
            with _handle(e) as c:
                elpd, se, dse, best = c.moments()
                w, f, gap, passes = c.stacking()
            elpd0, se0, dse0, best0 = r["moments"]
            tag = f"N={N} K={K} {kind} wgs={wgs}"
            rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))  # noqa: E731
            nz = dse0 > 0.0
            d_m = max(rel(elpd, elpd0), rel(se[se0 > 0], se0[se0 > 0]) if (se0 > 0).any() else 0.0, rel(dse[nz], dse0[nz]) if nz.any() else 0.0)
            gap_np = cr.kkt_gap(e, w)
            f_np = cr.objective(e, w)
            print(tag, "moments rel", d_m, "gap", gap, "passes", passes, "f - f_ref", f - r["f"], "max |w - w_ref|", np.abs(w - r["w"]).max())
            _note(f"moments/{kind}", rel=d_m)
            _note(f"stacking/{kind}", kkt_gap=max(gap, 0.0), passes=passes, gap_vs_numpy=abs(gap - gap_np),
                  objective_shortfall_per_N=max(r["f"] - f, 0.0) / N, objective_vs_numpy_rel=abs(f - f_np) / max(1.0, abs(f_np)))
            assert best == best0 and dse[best] == 0.0
            np.testing.assert_allclose(elpd, elpd0, rtol=1e-9, atol=0.0)
            np.testing.assert_allclose(se, se0, rtol=1e-9, atol=0.0)          # (N = 1: se = 0 on both sides)
            np.testing.assert_allclose(dse, dse0, rtol=1e-9, atol=0.0)
            assert np.all(w >= 0.0) and abs(w.sum() - 1.0) <= 1e-12, tag
            assert abs(gap - gap_np) <= 1e-9, (tag, gap, gap_np)
            assert gap <= 1e-8 and passes <= 64, (tag, gap, passes)
            assert abs(f - f_np) <= 1e-9 * max(1.0, abs(f_np)), (tag, f, f_np)
            assert f >= r["f"] - N * 1e-8 - 1e-9 * abs(r["f"]), (tag, f, r["f"])
            if kind != "dup":
                lam = r["lam"]
                bound = math.sqrt(2e-8 / lam) if lam > 0.0 else math.inf
                if math.isfinite(bound) and bound < 1.0:
                    _note(f"stacking/{kind}", weight_abs=np.abs(w - r["w"]).max())
                assert np.abs(w - r["w"]).max() <= bound, (tag, lam)


def test_permuted_rows_equal_prepermuted_rows(ref):
    e = ref(4097, 3, "close")["e"]
    order = np.random.default_rng(5).permutation(4097)
    with _handle(e) as a, _handle(e, order) as b:
        ma, mb = a.moments(), b.moments()
        sa, sb = a.stacking(), b.stacking()
        ba, bb = a.bb(9, 3, return_z=True), b.bb(9, 3, return_z=True)
    for x, y in zip(ma + sa + ba, mb + sb + bb):
        assert np.array_equal(x, y)


B_LIST = [1, 2, 7, 8, 9, 1000]


@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("N,K,kind", [(1, 2, "close"), (2, 3, "deep"), (63, 8, "dominant"), (65, 4, "dup"), (257, 3, "deep"), (1000, 4, "close"),
                                      (4097, 8, "close"), (4097, 2, "deep")])
def test_bootstrap_against_the_restatement(N, K, kind, wgs, ref, monkeypatch):
    _wgs(monkeypatch, wgs)
    r = ref(N, K, kind)
    e = r["e"]
    seed = 1234567890123 + N
    with _handle(e) as c:
        got = {B: c.bb(B, seed, return_z=True) for B in B_LIST}
        again = c.bb(1000, seed, return_z=True)
        other = c.bb(8, seed + 1, return_z=True)
    if 1000 not in r["bb"]:
        r["bb"][1000] = cr.bb(e, 1000, seed)
    z0, scale = r["bb"][1000][2], r["bb"][1000][3]
    for B in B_LIST:
        w, se, z = got[B]
        w0, se0 = cr.bb_finish(z0[:B])
        err = float(np.max(np.abs(z - z0[:B]) / scale[:B]))
        print(f"N={N} K={K} {kind} wgs={wgs} B={B}: z err / scale", err, "w err", np.abs(w - w0).max(), "se_bb rel", np.abs(se - se0).max() / max(se0.max(), 1e-300))
        _note(f"bb/{kind}", z_over_scale=err, weight_abs=np.abs(w - w0).max(), se_bb_rel=float(np.max(np.abs(se - se0) / np.maximum(se0, 1e-300))) if B > 1 and N > 1 else 0.0)
        assert np.all(np.abs(z - z0[:B]) <= 1e-9 * scale[:B])
        np.testing.assert_allclose(w, w0, rtol=0.0, atol=1e-9)
        if N > 1:
            np.testing.assert_allclose(se, se0, rtol=1e-9, atol=0.0)
        else:
            # one observation carries all the weight: z_bk = e_k whatever g is and se_bb is 0 in exact arithmetic -- both sides hold
            # only the last-bit rounding of (g e) / g, to which a relative bar does not apply: zero to 1e-9 of |e| on both sides
            assert np.all(se <= 1e-9 * np.abs(e[0])) and np.all(se0 <= 1e-9 * np.abs(e[0]))
        assert abs(w.sum() - 1.0) <= 1e-12
    assert np.array_equal(got[1000][2][:8], got[8][2]) and np.array_equal(got[9][2][:7], got[7][2])
    for x, y in zip(got[1000], again):
        assert np.array_equal(x, y)
    if N > 1:          # (one observation carries all the weight whatever it is)
        assert not np.array_equal(other[2], got[8][2])


def test_refusals(ref):
    from pymc_amd import _lib

    e = ref(65, 3, "close")["e"]
    with pytest.raises(ValueError, match="N >= 1 and 2 <= K <= 8"):
        cmp.Comparison(0, 3, device=0)
    with pytest.raises(ValueError, match="N >= 1 and 2 <= K <= 8"):
        cmp.Comparison(10, 1, device=0)
    with pytest.raises(ValueError, match="N >= 1 and 2 <= K <= 8"):
        cmp.Comparison(10, 9, device=0)
    with cmp.Comparison(65, 3, device=0) as c:
        c.set(0, e[:, 0])
        c.set(2, e[:, 2])
        for call in (c.moments, c.stacking, c.bb):
            with pytest.raises(ValueError, match="row 1 of 3 is not set"):
                call()
        with pytest.raises(ValueError, match="model 3 outside 0 .. 2"):
            c.set(3, e[:, 0])
        order = np.arange(65)
        order[7] = 8
        with pytest.raises(ValueError, match=r"order is not a permutation of 0 \.\. 64 \(entry 8 = 8\)"):
            c.set(1, e[:, 1], order)
        order[7] = 65
        with pytest.raises(ValueError, match=r"not a permutation.*entry 7 = 65"):
            c.set(1, e[:, 1], order)
        order[7] = -1
        with pytest.raises(ValueError, match=r"not a permutation.*entry 7 = -1"):
            c.set(1, e[:, 1], order)
        for bad, text in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
            x = e[:, 1].copy()
            x[40] = bad
            x[12] = bad
            with pytest.raises(ValueError, match=rf"model 1 has the non-finite value {text} at observation 12 "):
                c.set(1, x)
            with pytest.raises(ValueError, match=r"model 1 has the non-finite value .* at observation 3 "):
                c.set(1, x, np.roll(np.arange(65), 9))          # (order[j] = j - 9 mod 65: the offenders are observations 3 and 31)
        with pytest.raises(ValueError, match="row 1 of 3 is not set"):          # (the refused calls set nothing)
            c.moments()
        c.set(1, e[:, 1])
        for B in (0, -3, 65537):
            with pytest.raises(ValueError, match=rf"b_samples must lie in 1 \.\. 65536, not {B}"):
                c.bb(B, 0)
        w, se = c.bb(65536 // 64, 0)
        assert abs(w.sum() - 1.0) <= 1e-12
        assert c.moments()[3] == cr.moments(e)[3]
    assert _lib.load().nuts_compare_bb(None, 10, 0, None, None, None) == _lib.NUTS_E_ARG
    with pytest.raises(ValueError, match="model 1 has the non-finite value -inf at observation 5 "):
        cmp.compare_pointwise({"a": e[:, 0], "b": np.where(np.arange(65) == 5, -np.inf, e[:, 1])}, device=0)


def test_compare_pointwise_columns(ref):
    e = ref(1000, 4, "close")["e"]
    names = ["m0", "m1", "m2", "m3"]
    rows = {n: e[:, k] for k, n in enumerate(names)}
    elpd0, se0, dse0, best0 = cr.moments(e)
    rank = np.argsort(-elpd0, kind="stable")
    st = cmp.compare_pointwise(rows, p={"m1": 2.5}, warning={"m2": True}, device=0)
    assert st["names"] == [names[k] for k in rank] and np.array_equal(st["rank"], np.arange(4)) and st["scale"] == "log"
    np.testing.assert_allclose(st["elpd_loo"], elpd0[rank], rtol=1e-9)
    np.testing.assert_allclose(st["elpd_diff"], elpd0[best0] - elpd0[rank], rtol=1e-9, atol=1e-9 * abs(elpd0[best0]))
    assert st["elpd_diff"][0] == 0.0 and np.all(st["elpd_diff"] >= 0.0) and st["dse"][0] == 0.0
    np.testing.assert_allclose(st["se"], se0[rank], rtol=1e-9)
    np.testing.assert_allclose(st["dse"], dse0[rank], rtol=1e-9)
    assert st["p_loo"][st["names"].index("m1")] == 2.5 and np.isnan(st["p_loo"]).sum() == 3
    assert st["warning"] == [n == "m2" for n in st["names"]]
    assert st["kkt_gap"] <= 1e-10 and st["passes"] <= 18
    np.testing.assert_allclose(st["weight"], ref(1000, 4, "close")["w"][rank], atol=math.sqrt(2e-10 / ref(1000, 4, "close")["lam"]))
    bbr = cmp.compare_pointwise(rows, method="BB-pseudo-BMA", b_samples=64, seed=9, ic="waic", device=0)
    w0, se_bb0, _, _ = cr.bb(e, 64, 9)
    np.testing.assert_allclose(bbr["weight"], w0[rank], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(bbr["se"], se_bb0[rank], rtol=1e-9)
    assert "elpd_waic" in bbr and "p_waic" in bbr and "kkt_gap" not in bbr
    pb = cmp.compare_pointwise(rows, method="pseudo-BMA", device=0)
    np.testing.assert_allclose(pb["weight"], cr.pseudo_bma(elpd0)[rank], rtol=1e-9)


def _glm(X, y):
    m = ModelBuilder()
    alpha = m.Normal("alpha", 0.0, 5.0)
    beta = m.Normal("beta", 0.0, 1.0, shape=X.shape[1])
    m.GLM("y", X, beta, y, family="bernoulli", intercept=alpha, sigma=1.0)
    return m.build()


@pytest.mark.parametrize("ic,method", [("loo", "stacking"), ("loo", "BB-pseudo-BMA"), ("waic", "stacking")])
def test_compare_end_to_end(ic, method):
    """Two GLMs over the same 1 000 x 3 data, one with a covariate dropped, and a logit-rows model in unequal groups whose rows were
    passed unsorted (`rows_order` is not the identity); draws around the initial point, as tests/test_gpu_psis.py builds them."""
    rng = np.random.default_rng(21)
    X = rng.normal(size=(1000, 3)) / np.sqrt(3.0)
    y = (rng.random(1000) < 1.0 / (1.0 + np.exp(-(0.3 + X @ np.array([1.0, -0.5, 0.8]))))).astype("float64")
    rows_spec = rows_model([1, 370, 429, 200], 3, False)[0]
    assert rows_spec.rows_order is not None and not np.array_equal(np.asarray(rows_spec.rows_order), np.arange(1000))
    specs = {"glm3": _glm(X, y), "glm2": _glm(X[:, :2].copy(), y), "rows": rows_spec}
    S = 203
    models = {n: (s, np.random.default_rng(31 + k).normal(size=(1, S, s.n)) * 0.3) for k, (n, s) in enumerate(specs.items())}
    fn, col = (loglik.loo, "loo_i") if ic == "loo" else (loglik.waic, "waic_i")
    single = {n: fn(s, q, pointwise=True, device=0) for n, (s, q) in models.items()}
    got = cmp.compare(models, ic=ic, method=method, b_samples=16, seed=4, device=0)
    want = cmp.compare_pointwise({n: r[col] for n, r in single.items()}, method=method, b_samples=16, seed=4, ic=ic,
                                 p={n: r[f"p_{ic}"] for n, r in single.items()}, warning={n: r["warning"] for n, r in single.items()}, device=0)
    assert set(got) == set(want)
    for k in got:
        assert np.array_equal(got[k], want[k], equal_nan=True) if isinstance(got[k], np.ndarray) else got[k] == want[k], k
    elpd = np.array([single[n][f"elpd_{ic}"] for n in got["names"]])
    np.testing.assert_allclose(got[f"elpd_{ic}"], elpd, rtol=1e-9)
    assert np.all(np.diff(got[f"elpd_{ic}"]) <= 0.0) and got["elpd_diff"][0] == 0.0 and np.all(got["elpd_diff"] >= 0.0) and got["dse"][0] == 0.0
    assert abs(got["weight"].sum() - 1.0) <= 1e-12 and np.all(got["weight"] >= 0.0)
    np.testing.assert_allclose(got[f"p_{ic}"], [single[n][f"p_{ic}"] for n in got["names"]])
    with pytest.raises(ValueError, match="same number of observations"):
        cmp.compare({"glm3": models["glm3"], "short": (_glm(X[:500].copy(), y[:500]), np.zeros((1, 21, 4)))}, ic=ic, device=0)
