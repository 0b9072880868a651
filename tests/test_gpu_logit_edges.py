"""The row passes' own logistic (csrc/rows_kernel.h `logit_row`: exp, reciprocal and log1p written out for their narrow domain)
against mpmath at the edges of its domain, element by element, on every route that evaluates a single position.

Residuals: the isolating model of tests/logit_edges.py makes grad[mu_d] the residual r of ONE probe row with no rounding in
between, seven probes per evaluation (bit-exact on the oracle, tests/test_logit_edges.py); the probes sit in different groups (the
first and the last included), on a group's first row, rows 127 / 128 (the last row of a tile, the first row of the last tile) and
row 129 (the last valid row next to the masked padding).  Routes (each asserted by its model scalars): the span-partitioned general
pass, the group-aligned pass (forced), the same with the column of ones stored, the same with one wave per group, the group-block
pass, and the group-aligned pass with auxiliary workgroups.  Every route's r must stay within 16 max(1, E_O) in every regime, and
the routes must agree bit for bit, point by point.

All six routes run `logit_row`.  Its two-rows-side-by-side twin `logit_row2` is reached only by launches that evaluate the
positions of several chains at once (the interleaved path of `ga_tile` in rows_ga_multi_kernel.h for a group of two chains, and
rows_gal_kernel.h), which have no single-evaluation entry point; tests/test_gpu_chain_group.py holds those launches bitwise to the
single chain, i.e. to the arithmetic measured here (tried on a scratch build: one log1p coefficient of `logit_row2` changed in its
sixth digit passes this module and fails `test_grouped_chains_of_the_logit_rows_are_bitwise_the_chains_alone[64-130-2-20-8]` and
`test_the_lds_shared_kernel_is_bitwise_for_two_to_four_chains_too[64-130-2]`; one exp coefficient of `logit_row` changed the same
way fails 23 of the 28 tests here, the bitwise comparisons between routes excepted).

lp element-wise: `loglik.compute_log_likelihood` (k_ll_rows) on the same models with the evaluation points stacked as draws, in the
three row layouts; the probe rows within the bound, every filler row (eta = 0) the same double, within the bound of -ln 2.

lp in sum: at every evaluation point with |eta| <= 40, |logp_device - logp_mpmath| <= 16 sum_i den_i + K 2^-53 sum_i |t_i|
(den_i: the measure's denominator of row i; t_i: every term of the log-density, priors included, in mpmath; K = 64 for the
additions on the longest path of the reduction and the roundings inside a prior term together), and one dense case per route on rows of `models._hier_logit_data`
with eta spanning +-40.

GLM node, Bernoulli family (glm_kernel.h `glm_row` -> `logit_row`): beta ~ Flat, X = the 64 x 64 identity plus a zero row, so
grad[beta_p] = r_p; N = P = 1, so logp = lp.

With PYMC_AMD_LOGIT_EDGES_JSON set to a path, the run writes every regime's E_dev and every sum check's worst |miss| / bound there
(profiles/logit_edges.json).
"""
import contextlib
import json
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logit_edges as le  # noqa: E402

pytestmark = pytest.mark.gpu

SCHED_VARS = ("NUTS_ROWS_GA", "NUTS_ROWS_GB", "NUTS_GA_AUX", "NUTS_ROWS_GA_W", "NUTS_FOLD_CTL", "NUTS_LEAN_STRICT", "NUTS_GA_PACK", "NUTS_GA_ONES0")
GA = {"NUTS_ROWS_GA": "2"}
ROUTES = {
    "general": dict(G=20, rpg=60, env={}, expect={"rows_group_aligned": 0.0, "rows_group_block": 0.0, "lean": 1.0}),
    "ga": dict(G=12, rpg=130, env=GA, expect={"rows_group_aligned": 1.0, "rows_group_block": 0.0, "rows_aux_workgroups": 0.0}),
    "ga_ones_stored": dict(G=12, rpg=130, env={**GA, "NUTS_GA_ONES0": "0"}, expect={"rows_group_aligned": 1.0, "rows_group_block": 0.0, "rows_aux_workgroups": 0.0}),
    "ga_w1": dict(G=12, rpg=130, env={**GA, "NUTS_ROWS_GA_W": "1"}, expect={"rows_group_aligned": 1.0, "rows_group_block": 0.0, "rows_waves": 1.0}),
    "gb": dict(G=80, rpg=90, env={}, expect={"rows_group_aligned": 1.0, "rows_group_block": True}),
    "ga_aux": dict(G=12, rpg=130, env={**GA, "NUTS_GA_AUX": "1"}, expect={"rows_group_aligned": 1.0, "rows_group_block": 0.0, "rows_aux_workgroups": True}),
}
LOGLIK_ROUTES = ("general", "ga", "gb")          # the three row layouts of tests/test_gpu_loglik.py
ETA_SUM_MAX = 40.0

# K, the additions on the longest path from one row's lp to the log-density, read from the kernels:
#   general   rows_kernel.h `rows_main`: `lp += l` once per row of the lane, `wave_sum` (device_math.h: 6); kernels.h (kernel B):
#             `lp += lp_first`, one `lp += lg.wave_lp[w]` per further slice, `lp += ...` per element of the thread (its prior
#             terms), `wave_sum` (6), `t += s_w[w]` over the workgroup's waves, then the control kernel's sum over the workgroups'
#             partials in CTL_CHUNKS chunks;
#   ga / gb   rows_ga_kernel.h `ga_tile`: `lp += in ? l : 0` once per row of the lane, `wave_sum` into s_acc (6); `ga_tail_wave`:
#             `lpg += s_acc[ww][0][D] + s_acc[ww][1][D]` (2 W <= 8), `lpg += wave_sum(lpz)` (1 + 6), `ga_hyper_local` (1 + 6);
#             `ga_block_partial`: 8 records per chunk, then the chunks (<= 8); then the sum over the block partials and the
#             hyper-parameters' terms in the next prologue / the host read;
#   glm       glm_kernel.h `k_glm_rows`: `lp_acc += ...` per row of the lane, `wave_sum` (6), `t += s_part / s_sc` over 4 waves;
#             `k_glm_reduce`: `sum_strided` per chunk, `t += s_ch[c][cl]` over GLM_RED_CHUNKS = 64 chunks; then kernel B's path.
# Each of them is between 40 and some 80 at the shapes used here, so K is the cap the check allows, 64, and nothing is granted on
# top of it: the four roundings inside a prior term (-0.5 * r * r * inv_var - lognorm) count among the 64.
K_SUM = 64


@contextlib.contextmanager
def _route_env(env):
    keys = set(SCHED_VARS) | set(env)
    old = {k: os.environ.get(k) for k in keys}
    for k in keys:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _function(spec, expect):
    from pymc_amd.value_grad import DeviceValueGradFunction

    f = DeviceValueGradFunction(spec, device=0)
    for k, want in expect.items():
        got = f.model_scalar(k)
        ok = (got > 0) == (want > 0) if isinstance(want, bool) else got == want
        if not ok:
            f.close()
            raise AssertionError((k, got, want))
    return f


class _Runs:
    """runs[route][y] = dict(r over ETA, logp per chunk, ll [chunk, N] on the log-likelihood routes): a route's two models are built
    and evaluated when a test first asks for the route, so a route that fails its model scalars fails its own tests only"""

    def __init__(self):
        self._done = {}

    def __getitem__(self, route):
        if route not in self._done:
            self._done[route] = self._evaluate(route)
        return self._done[route]

    @staticmethod
    def _evaluate(route):
        from pymc_amd import loglik

        cfg, chunks, out = ROUTES[route], le.chunks(), {}
        with _route_env(cfg["env"]):
            for y in le.YS:
                spec, idx = le.rows_model(cfg["G"], cfg["rpg"], y)
                f = _function(spec, dict(cfg["expect"], rows_packed=0.0))          # (the one-hot X has far too many zeros to pack)
                try:
                    Q = np.stack([le.rows_point(cfg["G"], cfg["rpg"], ch) for ch in chunks])
                    r, logp = [], []
                    for q, ch in zip(Q, chunks):
                        lp, grad = f._pytensor_function(q)
                        r.append(le.read_residuals(grad, len(ch)))
                        logp.append(float(lp))
                    ll = loglik.compute_log_likelihood(spec, Q[None], func=f)["y"][0] if route in LOGLIK_ROUTES else None
                finally:
                    f.close()
                out[y] = dict(r=np.concatenate(r), logp=np.asarray(logp), ll=ll, idx=idx)
        return out


_runs = _Runs()


@pytest.fixture(scope="module")
def runs():
    return _runs


_profile = {"regimes": {}, "sum_checks": {}}


def _write_profile():
    path = os.environ.get("PYMC_AMD_LOGIT_EDGES_JSON")
    if path:
        with open(path, "w") as fh:
            json.dump(_profile, fh, indent=1, sort_keys=True)
            fh.write("\n")


def _record(values, errs, where, route):
    """into profiles/logit_edges.json, per regime and output: the oracle's error, the bound, the device's error with its worst point
    and the regime's largest absolute error (the worst over the routes), the routes measured, and whether they all gave that figure"""
    worst_abs = le.max_abs_errors(values)
    for k in errs:
        ent = _profile["regimes"].setdefault(k, {"E_O": le.E_O[k], "bound": le.bound(k), "cancelling": k.startswith("y1/pos/"), "E_dev": -1.0,
                                                 "max_abs_err": 0.0, "routes": [], "same_on_every_route": True})
        if ent["routes"] and errs[k] != ent["E_dev"]:
            ent["same_on_every_route"] = False
        if errs[k] > ent["E_dev"]:
            ent["E_dev"], ent["worst_eta"] = errs[k], where[k][0]
        ent["max_abs_err"] = max(ent["max_abs_err"], worst_abs[k])
        ent["routes"].append(route)
    _write_profile()


def _record_sum(what, route, ratio, per_row=None):
    """the worst |logp - truth| / bound of a sum check (and, for the dense case, the bound per row)"""
    ent = {"worst_miss_over_bound": ratio}
    if per_row is not None:
        ent["bound_per_row"] = per_row
    _profile["sum_checks"].setdefault(what, {})[route] = ent
    _write_profile()


def _assert_within(errs, where, what):
    for k in sorted(errs):
        print(f"{what} {k}: E_dev = {errs[k]:.4g}, E_O = {le.E_O[k]:.4g}, bound {le.bound(k):.4g}, worst at eta = {where[k][0]!r}")
    bad = {k: (e, le.bound(k), where[k][0]) for k, e in errs.items() if not e <= le.bound(k)}
    assert not bad, (what, bad)


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_residual_of_every_regime_is_within_its_bound(runs, route):
    values = {(y, "r"): runs[route][y]["r"] for y in le.YS}
    errs, where = le.regime_errors(values)
    assert set(errs) == {f"{k}/r" for k in le.REGIMES}
    _record(values, errs, where, route)
    _assert_within(errs, where, route)


@pytest.mark.parametrize("route", [r for r in ROUTES if r != "general"])
def test_the_residuals_of_all_routes_are_the_same_bits(runs, route):
    for y in le.YS:
        want, got = runs["general"][y]["r"], runs[route][y]["r"]
        diff = np.flatnonzero(got.view("u8") != want.view("u8"))          # (raw bits: the sign of a zero included)
        assert diff.size == 0, (route, y, [(float(le.ETA[i]), float(got[i]), float(want[i])) for i in diff[:5]])


@pytest.mark.parametrize("route", LOGLIK_ROUTES)
def test_the_pointwise_lp_of_every_regime_is_within_its_bound(runs, route):
    cfg = ROUTES[route]
    values = {}
    for y in le.YS:
        run = runs[route][y]
        ll, idx = run["ll"], run["idx"]
        assert ll.shape == (len(le.chunks()), cfg["G"] * cfg["rpg"])
        cols = [ll[s, idx[: len(ch)]] for s, ch in enumerate(le.chunks())]
        values[(y, "lp")] = np.concatenate(cols)
        # the filler rows (eta = 0, either y) and the probes beyond a short last chunk: ONE double, the device's lp at eta = 0
        filler = np.delete(ll, idx, axis=1)
        v0 = filler[0, 0]
        assert np.all(filler == v0), (route, y, np.unique(filler)[:4])
        assert np.all(ll[-1, idx[len(le.chunks()[-1]):]] == v0)
        for yy in le.YS:
            e = le.measure(float(v0), yy, 0.0, "lp")
            print(f"{route} filler rows: lp(eta = 0) = {float(v0)!r}, e = {e:.3g}")
            assert e <= le.bound(f"y{yy}/pos/tiny/lp")
    errs, where = le.regime_errors(values)
    assert set(errs) == {f"{k}/lp" for k in le.REGIMES}
    _record(values, errs, where, "loglik_" + route)
    _assert_within(errs, where, "loglik " + route)


def _sum_bound(den, tabs):
    return le.FACTOR * float(den) + K_SUM * 2.0 ** -53 * float(tabs)


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_summed_lp_of_the_isolating_model(runs, route):
    """|logp_device - logp_mpmath| <= 16 sum den_i + K 2^-53 sum |t_i| at every evaluation point with |eta| <= 40"""
    cfg = ROUTES[route]
    n, worst_all = 0, 0.0
    for y in le.YS:
        worst = 0.0
        for s, ch in enumerate(le.chunks()):
            if np.max(np.abs(ch)) > ETA_SUM_MAX:
                continue
            total, den, tabs = le.mp_rows_model_logp(cfg["G"], cfg["rpg"], y, tuple(float(e) for e in ch))
            lp = runs[route][y]["logp"][s]
            with mp.workprec(le.PREC):
                miss = float(abs(mp.mpf(lp) - total))
            worst = max(worst, miss / _sum_bound(den, tabs))
            assert miss <= _sum_bound(den, tabs), (route, y, ch.tolist(), lp, float(total), miss, _sum_bound(den, tabs))
            n += 1
        print(f"{route} y = {y}: worst |logp - truth| / bound = {worst:.3g}")
        worst_all = max(worst_all, worst)
    _record_sum("isolating", route, worst_all)
    assert n >= 60


@pytest.fixture(scope="module")
def dense_truths():
    return {}


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_summed_lp_on_dense_rows(dense_truths, route):
    """Rows of `models._hier_logit_data`, beta = z scaled so that eta spans +-40 (tests/logit_edges.py `dense_case`).  A wrong
    coefficient shifts every row the same way; the bound -- den_i enlarged by D ulp(eta_i) |r_i| for the kernel's own rounding of
    eta -- is 4 to 5e-14 per row at these sizes (asserted below: at most 5e-14), so that is the common shift this check resolves.
    Not 1e-14: 16 sum den_i is three quarters of it, and in den_i the cancelling regime's floor c = ulp(eta), 1e-15 to 7e-15 for the
    half of the rows with y = 1 and eta > 0; the reduction's share, K 2^-53 sum |t_i|, is about 1e-14 per row (asserted: at
    most 1.5e-14)."""
    cfg = ROUTES[route]
    key = (cfg["G"], cfg["rpg"])
    if key not in dense_truths:
        dense_truths[key] = le.dense_case(*key)
    spec, q, total, den, tabs = dense_truths[key]
    with _route_env(cfg["env"]):
        f = _function(spec, cfg["expect"])
        try:
            lp, _ = f._pytensor_function(q)
        finally:
            f.close()
    with mp.workprec(le.PREC):
        miss = float(abs(mp.mpf(float(lp)) - total))
    rows = cfg["G"] * cfg["rpg"]
    print(f"{route}: logp = {float(lp)!r}, |logp - truth| = {miss:.3g}, bound {_sum_bound(den, tabs):.3g} = {_sum_bound(den, tabs) / rows:.3g} per row")
    _record_sum("dense", route, miss / _sum_bound(den, tabs), _sum_bound(den, tabs) / rows)
    assert _sum_bound(den, tabs) <= 5e-14 * rows and K_SUM * 2.0 ** -53 * float(tabs) <= 1.5e-14 * rows
    assert miss <= _sum_bound(den, tabs)


# ---- GLM node, Bernoulli family --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def glm_runs():
    from pymc_amd.value_grad import DeviceValueGradFunction

    P = le.GLM_P
    pts = np.concatenate([le.ETA, np.zeros(-len(le.ETA) % P)])
    out = {}
    for y in le.YS:
        f = DeviceValueGradFunction(le.glm_model(P, y), device=0)
        try:
            res = [f._pytensor_function(ch) for ch in le.chunks(pts, P)]
        finally:
            f.close()
        f = DeviceValueGradFunction(le.glm_model(1, y), device=0)
        try:
            one = [f._pytensor_function(np.asarray([eta])) for eta in le.ETA]
        finally:
            f.close()
        out[y] = dict(r=np.concatenate([g for _, g in res])[: len(le.ETA)], logp=np.asarray([float(lp) for lp, _ in res]),
                      lp1=np.asarray([float(lp) for lp, _ in one]), r1=np.asarray([g[0] for _, g in one]), pts=pts)
    return out


def test_the_glm_node_is_within_its_bounds_and_agrees_with_the_rows(glm_runs, runs):
    """r through the 64-probe model and through N = P = 1, lp through N = P = 1 (logp IS the row's lp): within the bound per regime;
    all of it the bits of the row passes"""
    values = {(y, "r"): glm_runs[y]["r"] for y in le.YS}
    errs, where = le.regime_errors(values)
    _record(values, errs, where, "glm")
    _assert_within(errs, where, "glm")
    values = {(y, o): glm_runs[y][o + "1"] for y in le.YS for o in le.OUTPUTS}
    errs, where = le.regime_errors(values)
    assert set(errs) == set(le.E_O)
    _record(values, errs, where, "glm_one_row")
    _assert_within(errs, where, "glm one row")
    for y in le.YS:
        assert np.array_equal(glm_runs[y]["r"].view("u8"), runs["general"][y]["r"].view("u8"))          # (raw bits)
        assert np.array_equal(glm_runs[y]["r1"].view("u8"), runs["general"][y]["r"].view("u8"))


def test_the_summed_lp_of_the_glm_node(glm_runs):
    P = le.GLM_P
    n, worst = 0, 0.0
    for y in le.YS:
        for s, ch in enumerate(le.chunks(glm_runs[y]["pts"], P)):
            if np.max(np.abs(ch)) > ETA_SUM_MAX:
                continue
            with mp.workprec(le.PREC):
                terms = [le.truth(y, float(eta))[0] for eta in ch] + [le.truth(y, 0.0)[0]]          # (the all-zero row)
                den = sum(le.denominator(y, float(eta), "lp") for eta in ch) + le.denominator(y, 0.0, "lp")
                total, tabs = mp.fsum(terms), mp.fsum([abs(t) for t in terms])
                miss = float(abs(mp.mpf(glm_runs[y]["logp"][s]) - total))
            assert miss <= _sum_bound(den, tabs), (y, s, miss, _sum_bound(den, tabs))
            worst = max(worst, miss / _sum_bound(den, tabs))
            n += 1
    _record_sum("glm", "glm", worst)
    assert n >= 8
