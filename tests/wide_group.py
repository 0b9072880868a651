"""What the wide-chain-group tests share (tests/test_wide_group_host.py, tests/test_gpu_wide_group.py); needs no device.

The matrix-core launch of a wide chain group (pymc_amd/csrc/mvn_mfma_kernel.h: `k_mfm_pack` + `k_mvn_mfma_multi`) at the sizes
where its column loop changes shape, on MvNormal models with a NON-ZERO mean:

  * `SIZES`, `steps_per_wave`, `row_workgroups`: the loop `for (s = w; s < K / 16; s += 16)` under `#pragma unroll 4`, restated;
  * `model(k)`: the model, and (prec, mu, konst) bit for bit as the engine receives them (pymc_amd/value_grad.py, `build_mvn`);
  * `exact_logp`: the node's log-density of those doubles in exact integer / rational arithmetic, and `rounding_count(k)`, the
    constant of the bound the device is held to;
  * the members (seed, start point, generator) of every company the device tests form, the settings they are sampled under, and
    the CPU oracle's run of each member (oracle/ref_sampler.py), also over a mat-vec summed in another order.
"""
import functools
import math
import os
import sys
from fractions import Fraction

import numpy as np
import scipy.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# ---- the kernel's column loop, restated ------------------------------------------------------------------------------------------
MFM_WAVES = 16      # waves of a row workgroup; wave w takes the column steps w, w + 16, ... of K / 16
MFM_ROWS = 8        # rows of P per row workgroup
MFM_UNROLL = 4      # `#pragma unroll 4` over a wave's steps
MFM_CONTROL = 16    # control workgroups in front of the row workgroups

#   k     steps   per wave                                          row workgroups
#   16      1     wave 0: 1, waves 1 .. 15: none                     2 (behind 16 control workgroups)
#   48      3     waves 0 .. 2: 1, the others none                   6
#   240    15     waves 0 .. 14: 1, wave 15 none                     30
#   272    17     wave 0: 2, the others 1                            34
#   1040   65     wave 0: 5 (four unrolled + one), the others 4      130
SIZES = (16, 48, 240, 272, 1040)
MODEL_SEED = 5


def steps_per_wave(k):
    nsteps = k // 16
    return [len(range(w, nsteps, MFM_WAVES)) for w in range(MFM_WAVES)]


def row_workgroups(k):
    return (k + MFM_ROWS - 1) // MFM_ROWS


def leading(k):
    """Transitions from the start over which a chain on the matrix cores carries the oracle's integers (the bars of
    tests/test_gpu_chain_group.py: deeper trees at larger k, rounding reaches a U-turn test sooner)."""
    return 6 if k <= 512 else 2


# ---- the model -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model(k, seed=MODEL_SEED):
    """(spec, prec, mu, konst): `models.mvnormal`'s covariance with a mean of 3 N(0, 1); prec, mu and konst are the doubles the
    kernels read -- the lines of pymc_amd/value_grad.py (Cholesky, cho_solve, symmetrised, the log-determinant) and of `build_mvn`
    (csrc/engine.hip: konst = -0.5 k log(2 pi) - logdet) repeated."""
    from pymc_amd.model_spec import ModelBuilder

    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(k, k)))
    lam = np.logspace(np.log10(0.1), np.log10(10.0), k)
    cov = (Q * lam) @ Q.T
    cov = 0.5 * (cov + cov.T)
    mu = 3.0 * rng.normal(size=k)
    m = ModelBuilder()
    m.MvNormal("x", mu, cov)
    spec = m.build()
    mv = spec.mvnormal
    L = scipy.linalg.cholesky(mv.cov, lower=True)
    prec = np.ascontiguousarray(scipy.linalg.cho_solve((L, True), np.eye(len(mv.mu))))
    prec = 0.5 * (prec + prec.T)
    mu_e = np.ascontiguousarray(mv.mu, dtype="float64")
    logdet = float(np.log(np.diag(L)).sum())
    konst = -0.5 * k * math.log(2.0 * math.pi) - logdet
    assert np.any(mu_e != 0.0)
    return spec, prec, mu_e, konst


# ---- exact arithmetic ------------------------------------------------------------------------------------------------------------
def _mant_exp(a):
    """(M, ex): a == M * 2^ex element by element, M the 53-bit mantissas as int64."""
    a = np.asarray(a, dtype="float64")
    assert np.all(np.isfinite(a))
    m, ex = np.frexp(a)
    return np.ldexp(m, 53).astype(np.int64), ex.astype(np.int64) - 53       # (|m| < 1: exact)


def _common_exp(M, ex):
    nz = M != 0
    return int(ex[nz].min()) if np.any(nz) else 0


def _float_limbs(M, ex, e, L):
    """Signed L-bit limbs, as float64 arrays [limb, ...], of the integers N = M * 2^(ex - e): N == sum_t limbs[t] * 2^(L t)."""
    sh = np.where(M != 0, ex - e, 0).astype(np.int64)
    assert sh.min() >= 0
    sign = np.sign(M).astype("float64")
    A = np.abs(M).astype(np.uint64)
    nl = (53 + int(sh.max()) + L - 1) // L
    mask = np.uint64((1 << L) - 1)
    zero = np.uint64(0)
    out = np.empty((nl,) + M.shape)
    for t in range(nl):
        r = L * t - sh                                   # limb t = bits [r, r + L) of |M|
        down = A >> np.clip(r, 0, 63).astype(np.uint64)
        up = A << np.clip(-r, 0, 63).astype(np.uint64)   # (-r < L: the low L bits survive the wrap of uint64)
        v = np.where(r >= 0, np.where(r < 64, down, zero), np.where(-r < L, up, zero)) & mask
        out[t] = sign * v.astype("float64")
    return out


def _object_ints(M, ex, e):
    return np.array([int(m) << int(x - e) if m else 0 for m, x in zip(M.ravel().tolist(), ex.ravel().tolist())], dtype=object).reshape(M.shape)


def _pow2(e):
    return Fraction(1 << e, 1) if e >= 0 else Fraction(1, 1 << -e)


class ExactMvn:
    """-1/2 (q - mu)^T P (q - mu) + konst of the DOUBLES (P, mu, konst, q) without a rounding.  The doubles become integers over a
    common power of two and are cut into limbs of L bits with k (2^L - 1)^2 < 2^53: a matrix product of two limb arrays in float64
    is then exact in whatever order it is summed (every partial sum is an integer below 2^53), and the limb products are put together,
    and multiplied with d, as Python integers.  tests/test_wide_group_host.py holds it to plain `fractions.Fraction`."""

    def __init__(self, prec, mu, konst):
        self.prec = np.ascontiguousarray(prec, dtype="float64")
        self.mu = np.ascontiguousarray(mu, dtype="float64")
        self.konst = float(konst)
        self.k = len(self.mu)
        self.L = (53 - max(self.k - 1, 1).bit_length()) // 2
        assert self.k * ((1 << self.L) - 1) ** 2 < 1 << 53
        M, ex = _mant_exp(self.prec)
        self.ep = _common_exp(M, ex)
        self.Pl = _float_limbs(M, ex, self.ep, self.L)
        self.absP = np.abs(self.prec)

    def many(self, qs):
        """[(exact log-density as a Fraction, S = sum_ij |d_i| |P_ij| |d_j|)] of the positions qs [T][k].  S is formed in float64 from
        the exact d (relative error below (k + 3) 2^-53 < 2^-42: k + 3 < 2^11) and shrunk by 2^-40, so that a bound in terms of it is
        never wider than the one in terms of the true S."""
        qs = np.atleast_2d(np.asarray(qs, dtype="float64"))
        T, k, L = len(qs), self.k, self.L
        assert qs.shape == (T, k) and k + 3 < 1 << 11
        X = np.concatenate([qs, self.mu[None, :]])                      # [T + 1][k]: the positions, then mu
        M, ex = _mant_exp(X)
        e = _common_exp(M, ex)
        Xl = _float_limbs(M, ex, e, L)
        N = _object_ints(M, ex, e)
        ngroups = self.Pl.shape[0] + Xl.shape[0] - 1
        assert min(self.Pl.shape[0], Xl.shape[0]) < 1 << 9              # (a group's sum of parts stays inside int64)
        acc = np.zeros((ngroups, k, T + 1), dtype=np.int64)
        for s in range(self.Pl.shape[0]):
            for t in range(Xl.shape[0]):
                acc[s + t] += (self.Pl[s] @ Xl[t].T).astype(np.int64)   # exact
        Y = np.zeros((k, T + 1), dtype=object)
        for g in range(ngroups):
            Y += acc[g].astype(object) * (1 << (L * g))
        out = []
        for i in range(T):
            D = N[i] - N[T]
            y = Y[:, i] - Y[:, T]
            quad = Fraction(int(np.dot(D, y))) * _pow2(2 * e + self.ep)
            ad = np.array([float(abs(int(v)) * _pow2(e)) for v in D.tolist()])
            S = float(ad @ (self.absP @ ad)) * (1.0 - 2.0 ** -40)
            out.append((Fraction(-1, 2) * quad + Fraction(self.konst), S))
        return out

    def __call__(self, q):
        return self.many(np.asarray(q, dtype="float64")[None, :])[0]


_exact = {}


def exact_mvn(k):
    """`ExactMvn` of `model(k)` (the limbs of P are cut once)."""
    if k not in _exact:
        _, prec, mu, konst = model(k)
        _exact[k] = ExactMvn(prec, mu, konst)
    return _exact[k]


def exact_logp(q, prec, mu, konst):
    """(-1/2 sum_ij d_i P_ij d_j + konst as a `Fraction`, S = sum_ij |d_i| |P_ij| |d_j|), d = q - mu, of doubles taken as exact."""
    return ExactMvn(prec, mu, konst)(q)


def fraction_logp(q, prec, mu, konst):
    """The same in plain `fractions.Fraction`, product by product (k^2 of them: for small k)."""
    k = len(mu)
    d = [Fraction(float(q[i])) - Fraction(float(mu[i])) for i in range(k)]
    quad = Fraction(0)
    S = Fraction(0)
    for i in range(k):
        row = Fraction(0)
        arow = Fraction(0)
        for j in range(k):
            p = Fraction(float(prec[i, j]))
            row += p * d[j]
            arow += abs(p) * abs(d[j])
        quad += d[i] * row
        S += abs(d[i]) * arow
    return Fraction(-1, 2) * quad + Fraction(float(konst)), float(S)


# ---- the bound ---------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -53


def rounding_count(k):
    """C of |model_logp - exact| <= C 2^-53 S + 2^-52 |konst|: the roundings on the LONGEST path from one product P_ij d_j to the
    log-density of the draw, counted from the code (every one of them acts on a partial sum of magnitude <= S, most on far less;
    second-order terms are C^2 2^-106 S, nothing at C < 200):

      1            d_j = fl(q_j - mu_j)                                                      (`k_mfm_pack`)
      16 smax      a wave's accumulator: four MFMAs per column step, each adding four products in an order of the hardware's
                   choosing (<= 4 roundings), over the smax = ceil(K / 256) steps of wave 0 (`k_mvn_mfma_multi`, the stream)
      16           t += s_part[ww][r][w] over the sixteen waves (the first addition, to 0.0, is exact: counted all the same)
      1 + 1        fl(q_i - mu_i) once more on the left, and -0.5 (q_i - mu_i) * t: the halving is exact, the product rounds
                                                                                             (`mvm_tail_core`)
      3            `wave_sum8`: three DPP additions over the workgroup's eight rows
      ceil(nwg / 16) + 2 + 4
                   `mva_control` over the nwg = K / 8 records: a lane adds every sixteenth record in index order, two shuffle
                   additions pair the four record classes, the four waves are added in wave order
      1            `control_lean`: s_sum[PART_LP] + konst -- its rounding is at most 2^-53 (S / 2 + |konst|); the |konst| part
                   is the bound's second term

    The single-chain launch that evaluates a chain's START state (`k_mvn_aligned<8>`: 2 ceil(K / 512) fmas per lane, a wave sum of
    6, four waves, then the same tail and records) has a shorter path at every size, so a draw that stayed at the start is covered."""
    smax = max(steps_per_wave(k))
    nwg = row_workgroups(k)
    return 1 + 4 * MFM_UNROLL * smax + MFM_WAVES + 2 + 3 + ((nwg + 15) // 16 + 2 + 4) + 1


def bound(k, S, konst):
    return rounding_count(k) * U * S + 2.0 * U * abs(konst)


# ---- members, companies, settings ----------------------------------------------------------------------------------------------------
TUNE, DRAWS = 14, 6
ROUGH_SIZES = (48, 272)
ONE_SEEDS = 2                  # members 0 and 1 are the "two seeds" of the wide-of-one tests
COMPANY = {"five": 5, "sixteen": 16}

# a member's seed, by size and place; chosen on the CPU (tests/test_wide_group_host.py holds every property the device tests
# rely on: divergences inside a tree and the depth cap in the `rough` companies, integers that do not move when the oracle's
# mat-vec is summed in another order for the members compared with the oracle)
NARROW_SIZES = (24, 301)       # not multiples of 16: a group of such models does not become wide
SEEDS = {k: tuple(7000 + 37 * k + c for c in range(17)) for k in SIZES + NARROW_SIZES}   # (a 17th: the member a wide group refuses)


def step_kwargs(k, setting):
    if setting == "rough":
        return dict(step_scale=8.0, max_treedepth=4, early_max_treedepth=4)
    assert setting == "plain"
    return dict(max_treedepth=5) if k == 1040 else {}


def member(k, c):
    """(seed of the step, start point, seed of the chain's generator) of member c at size k -- the same in every company."""
    seed = SEEDS[k][c]
    _, _, mu, _ = model(k)
    start = mu + np.random.default_rng(seed + 100_000).normal(size=k)
    return seed, start, seed + 200_000


# ---- the oracle's run of a member ------------------------------------------------------------------------------------------------------
class PrecLogpGrad:
    """The node through the precision matrix, as the device evaluates it, with the mat-vec summed in ANOTHER order than
    numpy's: the columns reversed, or accumulated in extended precision."""

    def __init__(self, k, how):
        _, self.P, self.mu, self.konst = model(k)
        self.how = how
        if how == "reversed":
            self.Pr = np.ascontiguousarray(self.P[:, ::-1])
        elif how == "longdouble":
            self.Pl = self.P.astype(np.longdouble)
        else:
            raise ValueError(how)

    def __call__(self, q):
        d = np.asarray(q, dtype="float64") - self.mu
        if self.how == "reversed":
            t = self.Pr @ d[::-1].copy()
            lp = -0.5 * float(d[::-1] @ t[::-1]) + self.konst
        else:
            tl = self.Pl @ d.astype(np.longdouble)
            lp = float(-0.5 * (d.astype(np.longdouble) @ tl) + self.konst)
            t = tl.astype("float64")
        return lp, -t


@functools.lru_cache(maxsize=None)
def oracle_run(k, setting, c, how="spec", n=TUNE + DRAWS):
    """(draws [n, k], stats) of the first n transitions of member c's run (TUNE tuning transitions, then DRAWS) by the oracle sampler
    (oracle/ref_sampler.py `run_chain`) -- over the oracle's own restatement of the node (`how` = "spec": Cholesky solves,
    oracle/ref_models.py) or over `PrecLogpGrad`."""
    from oracle import ref_models, ref_sampler

    spec = model(k)[0]
    f = ref_models.SpecLogpGrad(spec) if how == "spec" else PrecLogpGrad(k, how)
    seed, start, gen = member(k, c)
    pot = ref_sampler.adapt_diag_potential([start], seed)
    step = ref_sampler.RefNUTS(f, k, potential=pot, rng=seed, **step_kwargs(k, setting))
    step.setup_chain(np.random.default_rng(gen), TUNE, DRAWS)
    step.tune = True
    step.reset_tuning()
    step.iter_count = 0
    q = np.asarray(start, dtype="d")
    out, stats = np.empty((n, k)), []
    for i in range(n):
        if i == TUNE:
            step.stop_tuning()
        q, st = step.astep(q)
        out[i] = q
        stats.append(st)
    return out, stats


INT_KEYS = ("depth", "tree_size", "index_in_trajectory", "diverging", "reached_max_treedepth")


def integers(stats, n):
    return [tuple(int(s[key]) for key in INT_KEYS) for s in stats[:n]]


@functools.lru_cache(maxsize=None)
def oracle_edge(k):
    """E_O of size k: the worst |lp_oracle - exact| / (2^-53 S) over every draw of the oracle's `plain` runs of members 0 and 1
    (the oracle's float64 log-density, `ref_models.SpecLogpGrad`, at its own draws)."""
    from oracle import ref_models

    f = ref_models.SpecLogpGrad(model(k)[0])
    worst = 0.0
    for c in range(ONE_SEEDS):
        draws, _ = oracle_run(k, "plain", c)
        for q, (ex, S) in zip(draws, exact_mvn(k).many(draws)):
            worst = max(worst, abs(float(Fraction(float(f(q)[0])) - ex)) / (U * S))
    return worst
