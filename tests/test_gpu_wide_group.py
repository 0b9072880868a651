"""The matrix-core launch of WIDE chain groups (csrc/mvn_mfma_kernel.h: `k_mfm_pack` + `k_mvn_mfma_multi`) at the sizes where its
column loop changes shape, on models with a non-zero mean, in companies of one, five and sixteen (tests/wide_group.py: the sizes, the
model, the members, the exact reference; tests/test_wide_group_host.py: what of it is held on the CPU).

A chain in a wide group is not bitwise the chain alone (the matrix instruction sums a row in another order), but column c of the
16 x 16 tile depends on chain c's own column of D only, in an order that does not depend on c: a member produces THE SAME BITS
whatever its company, its column in the launch and the number of chains the launch carries.  That is what holds this launch the way
"bitwise the chain alone" holds the others -- a race in `s_part`, in `dpack` (one buffer, consecutive launches) or in the handling of
`aborted` shows as a member that differs between two companies.  Against the outside: the oracle sampler's integers and the chain
alone over the leading transitions, and every draw's log-density against exact arithmetic, to a bound counted from the code.

All members go through the direct interface (`init_nuts` per member with its own start and generator, `sample_chain` per member, a
thread per member): `sample(chains=...)` starts the `adapt_diag` potential from the mean over ALL chains' starts, so its chain c is
another chain in a run of 6 and a run of 16.

Mutations tried on scratch builds (none committed), the 37 tests of this module run against each, and what caught them:
  * `k_mfm_pack` reading `mv.mu[k ^ 1]` -- 19 fail: all ten of `test_a_wide_group_of_one_follows_the_oracle_and_the_chain_alone` and
    nine of the ten `test_the_log_density_is_the_exact_one_to_the_counted_bound` (at k = 16 the two wide-of-one chains never leave
    their start, whose log-density the single-chain kernel evaluated); the bitwise comparisons pass: wrong, and the same in any company;
  * wave 0 starting its column steps at `w + 16` -- 22 fail: `test_a_wide_group_of_one_...` at every size and seed (k = 272 and k = 16
    among them), the bound of `test_the_log_density_...` in all ten cases, and two of the company comparisons;
  * no `__syncthreads()` between the `s_part` stores and the tail -- 15 fail: all seven of
    `test_a_member_is_the_same_bits_in_a_company_of_one_five_and_sixteen`, `test_members_of_different_length_leave_and_join_a_wide_group`,
    the bound in six cases (every sixteen-member run among them) and `test_a_wide_group_of_one_...[1040-1]`.
With PYMC_AMD_WIDE_GROUP_JSON set to a path, the run writes every size's worst E_dev = |model_logp - exact| / (2^-53 S), the constant C
and the oracle's E_O there (profiles/wide_group_edges.json).
"""
import json
import os
import sys
import threading
import time
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_group as wg  # noqa: E402
from test_gpu_chain_group import _same_stats  # noqa: E402

pytestmark = pytest.mark.gpu

WIDE = {"NUTS_MVN_ALIGNED": "8", "NUTS_GROUP_WIDE": "1"}
FOUR_ROWS = {"NUTS_MVN_ALIGNED": "4", "NUTS_GROUP_WIDE": "1"}


def _members(mp, k, setting, who, env=WIDE, tune=wg.TUNE):
    """[(start point, step, seed of the generator)] of the members `who`, their models and chains created under `env`."""
    from pymc_amd.sampling import init_nuts

    for key, value in env.items():
        mp.setenv(key, value)
    spec = wg.model(k)[0]
    out = []
    for c in who:
        seed, start, gen = wg.member(k, c)
        points, step = init_nuts(spec, init="adapt_diag", chains=1, random_seed_list=[seed], initvals={"x": start}, device=0, tune=tune,
                                 **wg.step_kwargs(k, setting))
        assert np.array_equal(points[0]["x"], start)
        out.append((points[0], step, gen))
    return out


def _sample_together(members, lengths, late=()):
    """`sample_chain` per member: on this thread when there is one, else on a thread each -- entering their first trees together,
    but for the members `late`, which start 20 ms behind.  [(draws, stats)] by member."""
    from pymc_amd.sampling import sample_chain

    if len(members) == 1:
        (start, st, gen), (tune, draws) = members[0], lengths[0]
        return [sample_chain(st, start, np.random.default_rng(gen), tune, draws)]
    res, err = [None] * len(members), []
    together = threading.Barrier(len(members) - len(late), timeout=120.0)

    def work(i):
        try:
            start, st, gen = members[i]
            st._logp_dlogp_func.bind_thread()
            if i in late:
                time.sleep(0.02)
            else:
                together.wait()
            res[i] = sample_chain(st, start, np.random.default_rng(gen), *lengths[i])
        except BaseException as e:   # noqa: BLE001 (reported by the caller's thread)
            err.append((i, e))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(len(members))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if err:
        raise err[0][1]
    return res


RUNS = {}


def _run(mp, k, setting, company):
    """The cached run of a company at size k: "one-c" (member c as a wide group of one), "alone-c" (member c with the same options
    and no group: `k_mvn_aligned<8>`), "five" (members 0 .. 4 as one wide group), "sixteen" (members 0 .. 15).
    dict(draws = {c: [transitions][k]}, stats = {c: [...]}, launches, wide_ok, aligned)."""
    from pymc_amd.chain_group import ChainGroup

    key = (k, setting, company)
    if key in RUNS:
        return RUNS[key]
    kind, _, c = company.partition("-")
    who = [int(c)] if c else list(range(wg.COMPANY[kind]))
    members = _members(mp, k, setting, who)
    group = None
    try:
        f = members[0][1]._logp_dlogp_func
        out = dict(wide_ok=f.model_scalar("chain_group_wide_ok"), aligned=f.model_scalar("mvn_row_aligned"))
        if kind != "alone":
            group = ChainGroup([st for _, st, _ in members])
        res = _sample_together(members, [(wg.TUNE, wg.DRAWS)] * len(members))
        out["launches"] = group.launches() if group else None
    finally:
        if group:
            group.close()
        for _, st, _ in members:
            st.close()
    out["draws"] = {c: r[0] for c, r in zip(who, res)}
    out["stats"] = {c: r[1] for c, r in zip(who, res)}
    RUNS[key] = out
    return out


# ---- (a) the route ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", wg.SIZES)
def test_a_group_of_one_is_wide_and_every_leapfrog_of_its_trees_a_matrix_core_launch(k, monkeypatch):
    run = _run(monkeypatch, k, "plain", "one-0")
    assert run["wide_ok"] == 1 and run["aligned"] == 8
    n = run["launches"]
    assert len(n) == 17, n                                         # (a group on the plain-fma kernels answers five entries)
    leapfrogs = sum(int(s["tree_size"]) for s in run["stats"][0])
    assert sum(n[2:]) == 0 and leapfrogs <= n[1] <= 1.5 * leapfrogs, (n, leapfrogs)   # (look-ahead launches drain behind a finished tree)
    for company in ("five", "sixteen"):
        assert len(_run(monkeypatch, k, "plain", company)["launches"]) == 17


# ---- (b) wide-of-one against the oracle and the chain alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("c", range(wg.ONE_SEEDS))
@pytest.mark.parametrize("k", wg.SIZES)
def test_a_wide_group_of_one_follows_the_oracle_and_the_chain_alone(k, c, monkeypatch):
    """One chain through `k_mvn_mfma_multi` with nc = 1 (column 0 of the tile, fifteen columns of zeros), every leapfrog of every
    tree, on one thread -- so nothing here depends on timing: the oracle sampler's integers over the leading transitions (which
    tests/test_wide_group_host.py shows not to hinge on the order of a sum), and the chain alone to rounding."""
    first = wg.leading(k)
    one, alone = _run(monkeypatch, k, "plain", f"one-{c}"), _run(monkeypatch, k, "plain", f"alone-{c}")
    assert alone["launches"] is None and alone["aligned"] == 8
    want = wg.integers(wg.oracle_run(k, "plain", c, "spec", first)[1], first)
    got = wg.integers(one["stats"][c], first)
    print(f"k = {k}, member {c}: (depth, tree_size, index_in_trajectory, diverging, reached_max_treedepth) {got}; the oracle's {want}")
    assert got == want
    assert wg.integers(alone["stats"][c], first) == want
    np.testing.assert_allclose(one["draws"][c][:first], alone["draws"][c][:first], rtol=1e-8, atol=1e-10)
    for i in range(first):
        for key in ("energy", "model_logp"):
            np.testing.assert_allclose(one["stats"][c][i][key], alone["stats"][c][i][key], rtol=1e-9, atol=1e-9, err_msg=f"{k} {c} {i} {key}")
    assert not np.array_equal(one["draws"][c][0], wg.member(k, c)[1])          # (the chain moved)


# ---- (c) company does not matter: bitwise ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,setting", [(k, "plain") for k in wg.SIZES] + [(k, "rough") for k in wg.ROUGH_SIZES])
def test_a_member_is_the_same_bits_in_a_company_of_one_five_and_sixteen(k, setting, monkeypatch):
    five, sixteen = _run(monkeypatch, k, setting, "five"), _run(monkeypatch, k, setting, "sixteen")
    n5, n16 = five["launches"], sixteen["launches"]
    print(f"k = {k}, {setting}: launches by chains carried, five members {n5[1:6]}, sixteen members {n16[1:]}")
    assert sum(n5[2:]) > 0 and sum(n5[6:]) == 0, n5                 # the larger companies really merged
    assert sum(n16[2:]) > 0 and sum(n16[5:]) > 0, n16
    for c in range(5):
        one = _run(monkeypatch, k, setting, f"one-{c}")
        for other, what in ((five, "five"), (sixteen, "sixteen")):
            assert np.array_equal(one["draws"][c], other["draws"][c]), (k, setting, c, what)
            _same_stats(one["stats"][c], other["stats"][c], (k, setting, c, what))
    for c in range(5, 16):          # (the eleven members that only the company of sixteen has)
        assert sixteen["draws"][c].shape == (wg.TUNE + wg.DRAWS, k) and np.all(np.isfinite(sixteen["draws"][c]))
    assert len({tuple(int(s["tree_size"]) for s in sixteen["stats"][c]) for c in range(16)}) > 1      # (trees of different shapes)
    if setting == "rough":
        for run, members in ((five, range(5)), (sixteen, range(16))):
            stats = [s for c in members for s in run["stats"][c]]
            assert any(s["diverging"] and int(s["tree_size"]) > 1 for s in stats)      # a tree that ended in a divergence: `dead` leaves in company
            assert any(s["reached_max_treedepth"] for s in stats)


# ---- (d) the log-density against exact arithmetic ------------------------------------------------------------------------------------------
EDGES = {}


def _record(k, e_dev):
    EDGES[k] = max(EDGES.get(k, 0.0), e_dev)
    path = os.environ.get("PYMC_AMD_WIDE_GROUP_JSON")
    if path:
        doc = {"bound": "|model_logp - exact| <= C 2^-53 S + 2^-52 |konst|; E = |miss| / (2^-53 S), worst over the draws",
               "sizes": {str(kk): {"E_dev": EDGES[kk], "C": wg.rounding_count(kk), "E_O": wg.oracle_edge(kk)} for kk in sorted(EDGES)}}
        with open(path, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


@pytest.mark.parametrize("company", ["one", "sixteen"])
@pytest.mark.parametrize("k", wg.SIZES)
def test_the_log_density_is_the_exact_one_to_the_counted_bound(k, company, monkeypatch):
    """Every draw of the wide-of-one runs and of the sixteen-member run: the `model_logp` the device recorded for the draw against
    -1/2 d^T P d + konst of the doubles the kernels read, in exact arithmetic, within C 2^-53 S + 2^-52 |konst| (tests/wide_group.py
    `rounding_count`: C counted from the code, 46 .. 118)."""
    konst = wg.model(k)[3]
    runs = [_run(monkeypatch, k, "plain", f"one-{c}") for c in range(wg.ONE_SEEDS)] if company == "one" else [_run(monkeypatch, k, "plain", "sixteen")]
    worst, fails = 0.0, []
    for run in runs:
        for c, draws in run["draws"].items():
            for i, (ex, S) in enumerate(wg.exact_mvn(k).many(draws)):
                miss = abs(float(Fraction(float(run["stats"][c][i]["model_logp"])) - ex))
                worst = max(worst, miss / (wg.U * S))
                if not miss <= wg.bound(k, S, konst):
                    fails.append((c, i, miss, wg.bound(k, S, konst)))
    print(f"k = {k}, {company}: worst E_dev = |model_logp - exact| / (2^-53 S) = {worst:.3f}; C = {wg.rounding_count(k)}")
    _record(k, worst)
    assert not fails, fails[:5]


# ---- (e) leaving and joining ---------------------------------------------------------------------------------------------------------------
def test_members_of_different_length_leave_and_join_a_wide_group(monkeypatch):
    """k = 272, six members, the lengths and the late start of the plain group's test (tests/test_gpu_chain_group.py): member 2 starts
    late and stops early, the others run on without it.  Each is bitwise its run as a wide group of one; and once the group is
    closed the chains are engines of their own again, bitwise as well."""
    from pymc_amd.chain_group import ChainGroup
    from pymc_amd.sampling import sample_chain

    k = 272
    lengths = [(20, 40), (40, 60), (10, 2), (20, 40), (30, 30), (12, 20)]

    def run(who, late):
        members = _members(monkeypatch, k, "plain", who, tune=30)
        group = ChainGroup([st for _, st, _ in members])
        try:
            res = _sample_together(members, [lengths[c] for c in who], late)
            n = group.launches()
            group.close()
            tail = [sample_chain(st, start, np.random.default_rng(7), 2, 3) for start, st, _ in members]
        finally:
            group.close()
            for _, st, _ in members:
                st.close()
        return res, tail, n

    res6, tail6, n6 = run(list(range(6)), (2,))
    assert len(n6) == 17 and sum(n6[2:]) > 0, n6
    for c in range(6):
        (res1,), (tail1,), n1 = run([c], ())
        assert sum(n1[2:]) == 0 and n1[1] > 0
        assert np.array_equal(res1[0], res6[c][0]), c
        _same_stats(res1[1], res6[c][1], c)
        assert np.array_equal(tail1[0], tail6[c][0]), c
        _same_stats(tail1[1], tail6[c][1], (c, "tail"))


# ---- (f) what does not become wide -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,env,wide_ok", [(24, WIDE, 0), (301, WIDE, 0), (48, FOUR_ROWS, None)])
def test_what_does_not_become_wide_stays_bitwise_the_chains_alone(k, env, wide_ok, monkeypatch):
    """k no multiple of 16, or a model laid out four rows per workgroup: the group its first member founds under NUTS_GROUP_WIDE = 1 is
    a plain one -- four chains at the most, on `k_mvn_aligned_multi`, bitwise the chains alone (non-zero mean included)."""
    from pymc_amd import _lib
    from pymc_amd.chain_group import ChainGroup

    lengths = [(wg.TUNE, wg.DRAWS)] * 4
    members = _members(monkeypatch, k, "plain", range(5), env)
    group = None
    try:
        f = members[0][1]._logp_dlogp_func
        if wide_ok is not None:
            assert f.model_scalar("chain_group_wide_ok") == wide_ok
        assert f.model_scalar("mvn_row_aligned") == int(env["NUTS_MVN_ALIGNED"])
        group = ChainGroup([st for _, st, _ in members[:4]])
        with pytest.raises(ValueError, match="a group holds at most 4 chains"):
            _lib.check(_lib.load().nuts_group_add(group._handle, members[4][1]._chain), "nuts_group_add")
        together = _sample_together(members[:4], lengths)
        n = group.launches()
        assert len(n) == 5 and sum(n[2:]) > 0, n
    finally:
        if group:
            group.close()
        for _, st, _ in members:
            st.close()
    for c in range(4):
        (alone,) = _alone(monkeypatch, k, env, c)
        assert np.array_equal(alone[0], together[c][0]), (k, c)
        _same_stats(alone[1], together[c][1], (k, c))


def _alone(mp, k, env, c):
    members = _members(mp, k, "plain", [c], env)
    try:
        return _sample_together(members, [(wg.TUNE, wg.DRAWS)])
    finally:
        members[0][1].close()


def test_a_wide_group_refuses_a_seventeenth_member(monkeypatch):
    from pymc_amd import _lib
    from pymc_amd.chain_group import ChainGroup

    members = _members(monkeypatch, 16, "plain", range(17))
    group = None
    try:
        group = ChainGroup([st for _, st, _ in members[:16]])
        assert len(group.launches()) == 17
        with pytest.raises(ValueError, match="a wide group holds at most 16 chains"):
            _lib.check(_lib.load().nuts_group_add(group._handle, members[16][1]._chain), "nuts_group_add")
    finally:
        if group:
            group.close()
        for _, st, _ in members:
            st.close()
