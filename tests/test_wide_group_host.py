"""What tests/test_gpu_wide_group.py relies on, held on the CPU (tests/wide_group.py): the sizes reach every shape of the matrix-core
launch's column loop, the exact reference is exact, the oracle sits well inside the bound the device is held to, the oracle's runs
contain the divergences and depth caps the device tests look for, and the oracle's integers over the transitions compared on the
device do not hinge on the order of a sum."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_group as wg  # noqa: E402


def test_the_sizes_reach_every_shape_of_the_column_loop():
    per = {k: wg.steps_per_wave(k) for k in wg.SIZES}
    for k, s in per.items():
        assert k % 16 == 0 and len(s) == wg.MFM_WAVES and sum(s) == k // 16, k
    assert any(0 in s for s in per.values())                                         # a wave with no step at all
    assert per[16] == [1] + [0] * 15                                                 # ... fifteen of them
    assert per[240] == [1] * 15 + [0]                                                # ... only the last one
    assert any(len(set(s)) > 1 and min(s) > 0 for s in per.values())                 # unequal counts, every wave at work
    assert per[272] == [2] + [1] * 15
    assert any(max(s) > wg.MFM_UNROLL and max(s) % wg.MFM_UNROLL == 1 for s in per.values())   # four unrolled steps plus one
    assert per[1040] == [5] + [4] * 15
    assert min(wg.row_workgroups(k) for k in wg.SIZES) == 2 == wg.row_workgroups(16)   # the smallest row grid
    assert wg.row_workgroups(1040) == 130
    # (the sizes the suite ran before: equal counts, at least one step, no remainder)
    for k in (256, 512, 1024, 2048):
        s = wg.steps_per_wave(k)
        assert len(set(s)) == 1 and s[0] >= 1 and (s[0] <= wg.MFM_UNROLL or s[0] % wg.MFM_UNROLL == 0)


def test_the_models_mean_is_not_zero_and_its_constants_are_the_engines():
    import math

    import scipy.linalg

    for k in wg.SIZES:
        spec, prec, mu, konst = wg.model(k)
        assert spec.n == k and np.count_nonzero(mu) == k and np.abs(mu).max() > 3.0
        assert np.array_equal(prec, prec.T)
        L = scipy.linalg.cholesky(spec.mvnormal.cov, lower=True)
        assert konst == -0.5 * k * math.log(2.0 * math.pi) - float(np.log(np.diag(L)).sum())
        np.testing.assert_allclose(prec @ spec.mvnormal.cov, np.eye(k), atol=1e-9)


@pytest.mark.parametrize("k", [16, 48, 240])
def test_the_exact_reference_is_plain_rational_arithmetic(k):
    """The limb-wise evaluation against `fractions.Fraction` product by product: the same rational number; S to its stated margin."""
    _, prec, mu, konst = wg.model(k)
    rng = np.random.default_rng(k)
    for q in (mu + rng.normal(size=k), mu + 1e-9 * rng.normal(size=k), 40.0 * rng.normal(size=k), mu.copy()):
        a, Sa = wg.exact_logp(q, prec, mu, konst)
        b, Sb = wg.fraction_logp(q, prec, mu, konst)
        assert a == b
        assert Sa <= Sb and Sb - Sa <= 2.0 ** -39 * Sb
    assert wg.exact_logp(mu, prec, mu, konst)[0] == Fraction(konst)


def test_the_bounds_constant_is_the_count_written_down():
    assert [wg.rounding_count(k) for k in wg.SIZES] == [46, 46, 47, 64, 118]


@pytest.mark.parametrize("k", wg.SIZES)
def test_the_oracle_sits_inside_the_bound_at_every_draw(k):
    """|lp_oracle - exact| <= C 2^-53 S + 2^-52 |konst| at every draw of the oracle's runs -- with room: the oracle's own error is
    a fraction of 2^-53 S (measured: 0.28, 0.14, 0.08 .. 0.12, 0.08, 0.02 .. 0.03 at k = 16 .. 1040; the last digits follow the host's
    BLAS)."""
    from oracle import ref_models

    spec, _, _, konst = wg.model(k)
    f = ref_models.SpecLogpGrad(spec)
    runs = [("plain", c) for c in range(wg.ONE_SEEDS)] + ([("rough", c) for c in range(5)] if k in wg.ROUGH_SIZES else [])
    worst = 0.0
    for setting, c in runs:
        draws, stats = wg.oracle_run(k, setting, c)
        for i, (q, (ex, S)) in enumerate(zip(draws, wg.exact_mvn(k).many(draws))):
            lp = f(q)[0]
            assert lp == stats[i]["model_logp"], (setting, c, i)          # (the log-density the oracle's sampler recorded for the draw)
            miss = abs(float(Fraction(float(lp)) - ex))
            worst = max(worst, miss / (wg.U * S))
            assert miss <= wg.bound(k, S, konst), (setting, c, i, miss, wg.bound(k, S, konst))
    print(f"k = {k}: worst |lp_oracle - exact| / (2^-53 S) = {worst:.3f}, C = {wg.rounding_count(k)}")
    assert wg.oracle_edge(k) <= worst


@pytest.mark.parametrize("k", wg.ROUGH_SIZES)
@pytest.mark.parametrize("company", sorted(wg.COMPANY))
def test_the_rough_companies_diverge_inside_a_tree_and_reach_the_depth_cap(k, company):
    """Ordinary sampler divergences that the oracle predicts: with a step eight times too long the first transitions of every member
    diverge, some of them after the tree has grown (its remaining leaves are the ones the launch sees as `dead`), and after tuning
    the trees stop at the cap of four doublings."""
    stats = [wg.oracle_run(k, "rough", c)[1] for c in range(wg.COMPANY[company])]
    mid = [(c, i, int(s["tree_size"])) for c, st in enumerate(stats) for i, s in enumerate(st) if s["diverging"] and int(s["tree_size"]) > 1]
    capped = [(c, i) for c, st in enumerate(stats) for i, s in enumerate(st) if s["reached_max_treedepth"]]
    assert mid and capped, (mid, capped)
    assert all(2 <= size <= 15 for _, _, size in mid)
    assert all(int(s["depth"]) <= 4 for st in stats for s in st)


@pytest.mark.parametrize("k", wg.SIZES)
def test_the_integers_compared_on_the_device_do_not_hinge_on_the_order_of_a_sum(k):
    """Members 0 and 1 under `plain`: the oracle's integers over the leading transitions (6 for k <= 512, 2 above) are the same when
    the node is evaluated through the precision matrix with the columns reversed, and accumulated in extended precision -- a device
    chain that departs from them is wrong, not unlucky."""
    first = wg.leading(k)
    for c in range(wg.ONE_SEEDS):
        want = wg.integers(wg.oracle_run(k, "plain", c)[1], first)
        assert len(want) == first
        for how in ("reversed", "longdouble"):
            got = wg.integers(wg.oracle_run(k, "plain", c, how, first)[1], first)
            assert got == want, (k, c, how, got, want)


def test_the_members_are_the_same_in_every_company():
    for k in wg.SIZES + wg.NARROW_SIZES:
        assert len(set(wg.SEEDS[k])) == 17
        a, b = wg.member(k, 3), wg.member(k, 3)
        assert a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])
        assert not np.array_equal(wg.member(k, 0)[1], wg.member(k, 1)[1])
    assert wg.step_kwargs(1040, "plain") == {"max_treedepth": 5} and wg.step_kwargs(272, "plain") == {}
    assert wg.step_kwargs(48, "rough") == {"step_scale": 8.0, "max_treedepth": 4, "early_max_treedepth": 4}
