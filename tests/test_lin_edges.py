"""The linear-predictor node at its shape edges, host side (tests/lin_edges.py; the device side is tests/test_gpu_lin_edges.py):
the exact reference against plain `fractions.Fraction`, the CPU oracle against the exact reference on every model the device runs
(bitwise on the integer family, inside the counted bound on the real-valued one -- the bound is not vacuous for a float64 evaluation
that is not the device's), and what the host says about columns with too many readers and with none."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lin_edges as le  # noqa: E402

from oracle import ref_models  # noqa: E402
from pymc_amd import model_spec as ms  # noqa: E402
from pymc_amd.model_spec import ModelBuilder  # noqa: E402

SMALL = {
    "two-readers": dict(N=5, P=3, K=2, readers=2),
    "some-columns": dict(N=6, P=2, K=3, readers=3, reader_cols=(0, 2)),
    "unread": dict(N=4, P=3, K=3, unread=(1,)),
    "derived": dict(N=4, P=3, coef="derived"),
    "shared": dict(N=3, P=4, N2=5),
    "one-row": dict(N=1, P=5, M=3, M2=4, readers=2),
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_exact_reference_is_plain_fraction_arithmetic(name):
    model = le.exact_model(**SMALL[name])
    for q in le.positions(model):
        ex = le.evaluate_exact(model, q)
        lik, grad = le.fraction_reference(model, q)
        assert ex.lik == lik, name
        assert ex.grad == grad, name
        assert all(g.denominator in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512) for g in grad)      # dyadic: a double holds it exactly


def test_the_reference_of_real_valued_doubles_is_plain_fraction_arithmetic():
    model = le.real_model(N=7, P=3, K=2, readers=2)
    for q in le.positions(model):
        ex = le.evaluate_exact(model, q)
        lik, grad = le.fraction_reference(model, q)
        assert ex.lik == lik and ex.grad == grad
        assert np.all(ex.S_grad >= np.abs(ex.grad_floats()) * (1 - 1e-9))       # S bounds what it is the absolute sum of


def test_the_device_list_reaches_every_edge_the_kernels_have():
    """The shapes of tests/test_gpu_lin_edges.py, restated against the kernels' constants: every KT full and partly filled, both
    sides of a forward workgroup and of a backward chunk, the forward grid's second trip, both limits, LIN_MAXUSE readers, and for
    the one-row kernels a trip that is full, one slot short, one slot over, and a second trip."""
    cases = le.EXACT_CASES
    ks = sorted({c.get("K", 1) for c in cases.values()})
    for kt in (1, 2, 4, 8, 16):
        assert any(le.kt_of(k) == kt for k in ks)
    for kt in (4, 8, 16):
        assert any(le.kt_of(k) == kt and k < kt for k in ks) and kt in ks
    ns = {c["N"] for c in cases.values()}
    for edge in (le.FWD_THREADS, le.LIN_CHUNK, 2 * le.LIN_CHUNK):
        assert {edge, edge + 1} <= ns
    assert {le.FWD_THREADS - 1, le.LIN_CHUNK - 1} <= ns and max(ns) > le.FWD_MAX_GRID * le.FWD_THREADS
    assert any(c["P"] == le.LIN_MAXP and c["N"] > 1 for c in cases.values())
    assert sum(1 for c in cases.values() if c["N"] > 1 and c["P"] * c.get("K", 1) == 4096) == 2
    assert max(c.get("readers", 1) for c in cases.values()) == le.LIN_MAXUSE
    one_row_p = {c["P"] for c in cases.values() if c["N"] == 1}
    one_row_m = {c.get("M") for c in cases.values() if c["N"] == 1}
    for s in (one_row_p, one_row_m):
        assert {le.ONE_ROW_TRIP, le.ONE_ROW_TRIP + 1, 1025, 1} <= s
    assert le.ONE_ROW_TRIP - 1 in one_row_p and 1023 in one_row_p and 1024 in one_row_p and max(one_row_p) > le.ONE_ROW_TRIP + 1024


@pytest.mark.parametrize("name", sorted(le.EXACT_CASES) + ["unread-column"])
def test_the_oracle_is_bitwise_exact_on_every_exact_model(name):
    model = le.exact_case(name)
    assert ms.engine_refusal(model.spec) is None and model.spec.lins
    C = le.logp_rounding_count(model)
    for q, ex in le.reference("exact", name):
        lp, g = ref_models.evaluate(model.spec, q)
        want = ex.grad_floats()
        assert all(float(f) == f for f in ex.grad[:64])                    # (the conversion to float64 is exact)
        assert np.array_equal(g, want), le.gradient_message(model, g, want)
        assert abs(lp - ex.logp_float()) <= le.bound(C, ex.S_logp), (name, lp, ex.logp_float())


@pytest.mark.parametrize("name", sorted(le.REAL_CASES))
def test_the_real_valued_oracle_stays_inside_the_counted_bound(name):
    model = le.real_case(name)
    assert ms.engine_refusal(model.spec) is None and model.spec.lins
    C, Cl = le.rounding_count(model), le.logp_rounding_count(model)
    for q, ex in le.reference("real", name):
        lp, g = ref_models.evaluate(model.spec, q)
        err = np.abs(g - ex.grad_floats())
        lim = le.bound(C, ex.S_grad) + le.U * np.abs(ex.grad_floats())       # (+ the reference's own conversion to float64)
        assert np.all(err <= lim), (name, int(np.argmax(err / lim)), float(np.max(err / lim)))
        assert np.any(err > 0) and np.all(lim < 1e-9 * np.maximum(1.0, np.max(np.abs(g))))      # neither vacuous nor trivially met
        assert abs(lp - ex.logp_float()) <= le.bound(Cl, ex.S_logp) + le.U * abs(lp), (name, lp, ex.logp_float())


def test_the_counts_are_what_the_kernels_say():
    """`rounding_count` written out for three models (the counts in its docstring, added by hand)."""
    m = le.exact_model(N=2049, P=3, K=5, readers=3)
    #      forward P   y - eta   lin_adj   8 fmas + wave + 4 waves + 2 chunks + n_src   prior, gdense, chain rule
    assert le.rounding_count(m) == 3 + 1 + 2 + (8 + 6 + 4 + 2 + 1) + (3 + 1 + 2)
    m = le.real_model(N=300, P=512, K=8, coef="log")
    assert le.rounding_count(m) == 2 + 512 + 1 + 0 + (8 + 6 + 4 + 1 + 1) + (3 + 1 + 2 + 2)
    m = le.real_model(N=1, P=9217, M=7)
    #      10 fmas + wave + 16 waves   y - eta   1 addition + wave + 16 waves + x * total + n_src
    assert le.rounding_count(m) == (10 + 6 + 16) + 1 + (1 + 6 + 16 + 1 + 1) + (3 + 1 + 2)


# ---- what the host says about a column's readers -------------------------------------------------------------------------------------
def test_a_column_with_five_readers_is_refused_in_the_engines_words():
    assert ms.LIN_MAXUSE == le.LIN_MAXUSE
    assert ms.engine_refusal(le.exact_model(N=8, P=2, readers=4).spec) is None
    assert ms.engine_refusal(le.exact_model(N=8, P=2, K=3, readers=4).spec) is None
    msg = ms.engine_refusal(le.exact_model(N=8, P=2, readers=5).spec)
    assert msg == "a linear predictor column is read by too many factors (LIN_MAXUSE)"      # csrc/engine.hip `build_lins`
    # one column of three with a fifth reader is enough; a factor that names a column twice reads it once (`add_lin`)
    assert "read by too many factors" in ms.engine_refusal(le.exact_model(N=8, P=2, K=3, readers=5, reader_cols=(1,)).spec)
    m = ModelBuilder()
    b = m.Normal("b", 0.0, 1.0, shape=2)
    eta = m.dot(np.arange(8.0).reshape(4, 2), b)
    for r in range(4):
        m.Potential(f"r{r}", eta * eta + eta)
    assert ms.engine_refusal(m.build()) is None


@pytest.mark.parametrize("n_unread", [4, 3])
def test_a_predictor_no_factor_reads_is_accepted_and_adds_nothing(n_unread):
    """Host side of the unread-column fix (pymc_amd/csrc/lin_kernel.h `lin_adj`, engine.hip `launch_vector`): the spec is accepted,
    the unread predictor contributes no gradient, and its Deterministic is evaluated on the host."""
    spec, X, Xu = le.deterministic_model(n_unread)
    assert ms.engine_refusal(spec) is None and len(spec.lins) == 2
    for q in (np.zeros(3), np.array([0.5, -1.0, 2.0]), np.array([-0.125, 1.75, 0.25])):
        lp, g = ref_models.evaluate(spec, q)
        assert np.array_equal(g, X.T @ (0.0 - X @ q) - q)                    # small dyadic numbers: exact in float64
        prog, term, size = spec.deterministics["eta2"]
        assert size == n_unread and np.array_equal(ms.eval_program(spec, prog, term, q), 2.0 * (Xu @ q))


def test_an_unread_column_gets_the_priors_gradient_only():
    model = le.exact_case("unread-column")
    K = model.K
    for q, ex in le.reference("exact", "unread-column"):
        g = ex.grad_floats().reshape(model.P, K)
        assert np.array_equal(g[:, 2], -q.reshape(model.P, K)[:, 2])
        assert np.any(g[:, :2] != -q.reshape(model.P, K)[:, :2])      # (the read columns do get the likelihood's share)
