"""NumPy restatement of the model comparison (pymc_amd/csrc/compare.h; `az.compare` on the log scale).

  moments        elpd_k = sum_i e_ik, se_k = sqrt(N var_pop(e_.k)), dse_k = sqrt(N var_pop(e_.best - e_.k)), best = argmax elpd
  stacking       Yao, Vehtari, Simpson, Gelman, "Using stacking to average Bayesian predictive distributions", Bayesian Analysis 13
                 (2018): maximise f(w) = sum_i log sum_k w_k exp(e_ik) over the simplex.  Terms shifted per observation,
                 m_i = max_k e_ik, p_ik = exp(e_ik - m_i): f(w) = sum_i [m_i + log sum_k w_k p_ik].  `solve` is the solver of the header;
                 `slsqp` is ArviZ's own formulation (K - 1 free weights, SLSQP with its gradient) on the same shifted terms.
  BB-pseudo-BMA  the Bayesian bootstrap of Yao et al. section 3.4: replicate b weighs the observations by Dirichlet(1, ..., 1) =
                 g(b, .) / sum_j g(b, j), g = -log u an Exp(1) variate from Philox (tests/predictive_reference.py):
                 key = (seed low, seed high), counter = (i low, i high, b >> 1, 0xFFFF0000), even b takes u0, odd b u1.
                 z_bk = N sum_i g(b, i) e_ik / sum_i g(b, i); weight_k = mean_b softmax_k(z_bk); se_bb_k = std_pop_b(z_bk).
"""
import math

import numpy as np

import predictive_reference as ppr

TAG = 0xFFFF0000          # kind 3, index 0x3fff, t = 0
KINDS = ("close", "dominant", "deep", "dup")
N_LIST = (1, 2, 63, 64, 65, 257, 1000, 4097)
K_LIST = (2, 3, 4, 8)


def make(N, K, seed, kind):
    rng = np.random.default_rng(seed)
    base = -1.0 + 0.8 * rng.standard_normal(N)
    if kind == "deep":
        return -700.0 + 50.0 * rng.standard_normal((N, K))
    e = base[:, None] + 0.3 * rng.standard_normal((N, K))
    if kind == "dominant":
        e[:, 0] += 1.0
    elif kind == "dup":
        e[:, K - 1] = e[:, 0]
    else:
        assert kind == "close", kind
    return e


def grid():
    """(N, K, kind, seed) of every input of the tests"""
    return [(N, K, kind, 1000 * N + 10 * K + j) for N in N_LIST for K in K_LIST for j, kind in enumerate(KINDS)]


# ---- moments ---------------------------------------------------------------------------------------------------------------------------
def moments(e):
    N = e.shape[0]
    elpd = e.sum(axis=0)
    best = int(np.argmax(elpd))
    se = np.sqrt(N * np.var(e, axis=0))
    dse = np.sqrt(N * np.var(e[:, [best]] - e, axis=0))
    return elpd, se, dse, best


# ---- stacking ---------------------------------------------------------------------------------------------------------------------------
def terms(e):
    m = e.max(axis=1)
    return m, np.exp(e - m[:, None])


def stack_pass(p, w):
    """sum_i log d_i, g, H at w (d_i = sum_k w_k p_ik)"""
    N = p.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = p @ w
        q = p / d[:, None]
        return float(np.log(d).sum()), q.sum(axis=0) / N, -(q.T @ q) / N


def min_norm_solve(A, b, cut=1e-10):
    """x of least norm minimising |A x - b| for symmetric A, eigen-directions below `cut` of the largest |eigenvalue| dropped"""
    lam, V = np.linalg.eigh(A)
    keep = np.abs(lam) > cut * np.abs(lam).max()
    return V[:, keep] @ ((V[:, keep].T @ b) / lam[keep])


def newton_direction(w, g, H):
    """the step of the equality-constrained Newton system on the free face; zero where pinned"""
    K = w.size
    free = (w > 0.0) | (g > 1.0)
    while True:
        F = np.flatnonzero(free)
        nf = F.size
        A = np.zeros((nf + 1, nf + 1))
        A[:nf, :nf] = H[np.ix_(F, F)]
        A[:nf, nf] = A[nf, :nf] = 1.0
        rhs = np.concatenate([-g[F], [0.0]])
        delta = np.zeros(K)
        delta[F] = min_norm_solve(A, rhs)[:nf]
        stuck = free & (w <= 0.0) & (delta <= 0.0)       # a freed weight that would leave the simplex: pinned after all
        if not stuck.any():
            return delta
        free &= ~stuck


HALVINGS = 6


def solve(e, tol=1e-12, max_passes=64):
    """-> w, f(w), kkt_gap, passes"""
    N, K = e.shape
    m, p = terms(e)
    sm = float(m.sum())
    w = np.full(K, 1.0 / K)
    ld, g, H = stack_pass(p, w)
    passes = 1
    while True:
        gap = float(g.max() - 1.0)
        if gap <= tol or passes >= max_passes:
            break
        delta = newton_direction(w, g, H)
        accepted = False
        if np.any(delta != 0.0):
            alpha, hit = 1.0, -1
            for k in range(K):
                if delta[k] < 0.0 and -w[k] / delta[k] < alpha:
                    alpha, hit = -w[k] / delta[k], k
            slack = 1e-13 * max(1.0, abs(ld))
            for h in range(HALVINGS):
                if passes >= max_passes:
                    break
                wn = np.maximum(w + alpha * delta, 0.0)
                if h == 0 and hit >= 0:
                    wn[hit] = 0.0
                wn = wn / wn.sum()
                ldn, gn, Hn = stack_pass(p, wn)
                passes += 1
                if np.isfinite(ldn) and ldn >= ld - slack:
                    w, ld, g, H, accepted = wn, ldn, gn, Hn, True
                    break
                alpha *= 0.5
        if not accepted and passes < max_passes:
            wn = w * g
            w = wn / wn.sum()
            ld, g, H = stack_pass(p, w)
            passes += 1
    return w, sm + ld, float(g.max() - 1.0), passes


def objective(e, w):
    m, p = terms(e)
    return float(m.sum() + np.log(p @ w).sum())


def kkt_gap(e, w):
    _, p = terms(e)
    return float(stack_pass(p, np.asarray(w, dtype="float64"))[1].max() - 1.0)


def curvature(e, w):
    """the smallest eigenvalue of -H on the sum-zero directions at w"""
    _, p = terms(e)
    H = stack_pass(p, w)[2]
    K = w.size
    Q = np.linalg.qr(np.column_stack([np.ones(K), np.eye(K)[:, :K - 1]]))[0][:, 1:]
    return float(np.linalg.eigvalsh(Q.T @ (-H) @ Q).min())


def slsqp(e):
    """ArviZ's `_stacking` formulation on the shifted terms -> w, f(w)"""
    from scipy.optimize import minimize

    N, K = e.shape
    m, p = terms(e)

    def full(w):
        return np.concatenate((w, [max(1.0 - np.sum(w), 0.0)]))

    def score(w):
        return -np.sum(np.log(p @ full(w)))

    def grad(w):
        d = p @ full(w)
        return -np.array([np.sum((p[:, k] - p[:, K - 1]) / d) for k in range(K - 1)])

    res = minimize(fun=score, x0=np.full(K - 1, 1.0 / K), jac=grad, bounds=[(0.0, 1.0)] * (K - 1),
                   constraints=[{"type": "ineq", "fun": lambda x: 1.0 - np.sum(x)}, {"type": "ineq", "fun": np.sum}])
    w = full(res.x)
    w = np.maximum(w, 0.0)
    w = w / w.sum()
    return w, objective(e, w)


# ---- Bayesian bootstrap ------------------------------------------------------------------------------------------------------------------
def bb_variates(seed, b, i, libm=False):
    """g(b, i) over the broadcast of b and i.  u is exact; NumPy's vectorised log may differ from the C library's in the last bit, so
    `libm` takes the logarithm element by element through math.log (what a host build of the header calls)."""
    b, i = np.broadcast_arrays(np.asarray(b, dtype=np.uint64), np.asarray(i, dtype=np.uint64))
    seed = int(seed)
    w = ppr.philox((i & ppr.MASK, i >> ppr.SH, b >> np.uint64(1), np.uint64(TAG)), (seed & 0xFFFFFFFF, seed >> 32))
    u = np.where((b & np.uint64(1)) == 0, ppr.u53(w[0], w[1]), ppr.u53(w[2], w[3]))
    if libm:
        return -np.vectorize(math.log, otypes=[float])(u)
    return -np.log(u)


def bb(e, b_samples, seed, block=64):
    """-> weights [K], se_bb [K], z [B][K], scale [B][K] (= N sum_i g |e_ik| / sum_i g: what the rounding of z_bk is relative to)"""
    N, K = e.shape
    z = np.empty((b_samples, K))
    scale = np.empty((b_samples, K))
    idx = np.arange(N, dtype=np.uint64)
    for b0 in range(0, b_samples, block):
        bs = np.arange(b0, min(b0 + block, b_samples), dtype=np.uint64)
        g = bb_variates(seed, bs[:, None], idx[None, :])
        tot = g.sum(axis=1)
        z[b0:b0 + bs.size] = N * (g @ e) / tot[:, None]
        scale[b0:b0 + bs.size] = N * (g @ np.abs(e)) / tot[:, None]
    return bb_finish(z) + (z, scale)


def bb_finish(z):
    u = np.exp(z - z.max(axis=1, keepdims=True))
    return (u / u.sum(axis=1, keepdims=True)).mean(axis=0), z.std(axis=0)


def pseudo_bma(elpd):
    u = np.exp(elpd - elpd.max())
    return u / u.sum()
