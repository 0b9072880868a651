"""NumPy restatement of the posterior-predictive variates (pymc_amd/csrc/predictive.h), from the papers:

  Philox4x32-10    Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11 (section 3.3, table 2: the
                   multipliers and Weyl key increments)
  Box-Muller       z = sqrt(-2 log u0) cos(2 pi u1)
  gamma            Marsaglia & Tsang, "A simple method for generating gamma variables", ACM TOMS 26 (2000), without the squeeze;
                   shape < 1 through gamma(a + 1) u^(1 / a) (their section 6)
  Poisson, mu < 10 sequential search from one uniform (Devroye, "Non-uniform random variate generation", X.3.3)
  Poisson, mu >= 10 Hormann, "The transformed rejection method for generating Poisson random variables", 1993 (algorithm PTRS)

The value of (draw s, observation i) of node (kind, index) under `seed` reads the blocks counter = (i low, i high, s, tag | t) under
key = (seed low, seed high), tag = kind << 30 | index << 16; a block gives two doubles u0 = U(w0, w1), u1 = U(w2, w3),
U(lo, hi) = ((hi >> 5) 2^26 + (lo >> 6) + 0.5) 2^-53.  Everything is vectorised over broadcast arrays of (s, i).

Every discrete result comes with its DECISION MARGIN: the smallest |lhs - rhs| over the comparisons that decided it (and the
distance of a floor's argument to the integers): an implementation whose libm rounds differently may decide an element with a
tiny margin the other way.
"""
import numpy as np
from scipy.special import expit, gammaln

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SH = np.uint64(32)

(D_NORMAL, D_HALFNORMAL, D_CAUCHY, D_HALFCAUCHY, D_STUDENTT, D_BETA, D_EXPONENTIAL, D_UNIFORM, D_BERNOULLI_LOGIT, D_LOGNORMAL,
 D_BERNOULLI, D_TRUNCNORMAL, D_POTENTIAL, D_BINOMIAL, D_GAMMA, D_INVGAMMA, D_LAPLACE, D_POISSON, D_DERIVED) = range(19)

GAMMA_TRIES, PTRS_TRIES, POIS_KMAX, T_BLOCK = 32, 64, 1000, 128


def philox(ctr, key):
    """ctr: four uint32 arrays (broadcastable), key: two -> four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> SH) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> SH) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def u53(lo, hi):
    return ((hi >> np.uint32(5)).astype("float64") * 2.0 ** 26 + (lo >> np.uint32(6)).astype("float64") + 0.5) * 2.0 ** -53


class Address:
    """(seed, node, draws s, observations i): block(t) -> (u0, u1) over the broadcast of s and i"""

    def __init__(self, seed, kind, index, s, i):
        assert 0 <= kind <= 3 and 0 <= index <= 0x3FFF
        seed = int(seed)
        self.key = (seed & 0xFFFFFFFF, seed >> 32)
        self.tag = kind << 30 | index << 16
        self.s, self.i = np.broadcast_arrays(np.asarray(s, dtype=np.uint64), np.asarray(i, dtype=np.uint64))
        self.shape = self.s.shape

    def sub(self, mask):
        a = object.__new__(Address)
        a.key, a.tag, a.s, a.i, a.shape = self.key, self.tag, self.s[mask], self.i[mask], (int(mask.sum()),)
        return a

    def block(self, t):
        assert 0 <= t < 65536
        w = philox((self.i & MASK, self.i >> SH, self.s, np.uint64(self.tag | t)), self.key)
        return u53(w[0], w[1]), u53(w[2], w[3])

    def normal(self, t):
        u0, u1 = self.block(t)
        return np.sqrt(-2.0 * np.log(u0)) * np.cos(2.0 * np.pi * u1)


def gamma(a, adr, t0):
    """standard gamma of shape a (array of adr.shape), blocks t0 .. t0 + 63; NaN after 32 rejections"""
    a = np.broadcast_to(np.asarray(a, dtype="float64"), adr.shape)
    out = np.full(adr.shape, np.nan)
    todo = np.ones(adr.shape, dtype=bool)
    a1 = np.where(a < 1.0, a + 1.0, a)
    d = a1 - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    for j in range(GAMMA_TRIES):
        if not todo.any():
            break
        sub = adr.sub(todo)
        x = sub.normal(t0 + 2 * j)
        u, u2 = sub.block(t0 + 2 * j + 1)
        dd, aa = d[todo], a[todo]
        w = 1.0 + c[todo] * x
        v = w * w * w
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = (v > 0.0) & (np.log(u) < 0.5 * x * x + dd - dd * v + dd * np.log(v))
            g = dd * v
            g = np.where(aa < 1.0, g * np.exp(np.log(u2) / aa), g)
        idx = np.flatnonzero(todo.ravel())[ok]
        out.ravel()[idx] = g[ok]
        todo.ravel()[idx] = False
    return out


def poisson(mu, adr):
    """-> (k, margin)"""
    mu = np.broadcast_to(np.asarray(mu, dtype="float64"), adr.shape)
    out = np.full(adr.shape, np.nan)
    margin = np.full(adr.shape, np.inf)
    small = mu < 10.0
    if small.any():
        sub = adr.sub(small)
        m = mu[small]
        u = sub.block(0)[0]
        k = np.zeros(m.shape)
        p = np.exp(-m)
        s = p.copy()
        mg = np.abs(u - s)
        live = u > s
        while live.any():
            live &= k < POIS_KMAX
            k = np.where(live, k + 1.0, k)
            p = np.where(live, p * m / np.maximum(k, 1.0), p)
            s = np.where(live, s + p, s)
            mg = np.where(live, np.minimum(mg, np.abs(u - s)), mg)
            live &= u > s
        out[small] = k
        margin[small] = mg
    big = ~small & np.isfinite(mu)
    if big.any():
        ob, mb = np.full(int(big.sum()), np.nan), np.full(int(big.sum()), np.inf)
        todo = np.ones(ob.shape, dtype=bool)
        base = adr.sub(big)
        mm = mu[big]
        for j in range(PTRS_TRIES):
            if not todo.any():
                break
            sub = base.sub(todo)
            m = mm[todo]
            mg = mb[todo]
            smu = np.sqrt(m)
            b = 0.931 + 2.53 * smu
            a = -0.059 + 0.02483 * b
            inv_alpha = 1.1239 + 1.1328 / (b - 3.4)
            vr = 0.9277 - 3.6224 / (b - 2.0)
            u0, V = sub.block(j)
            U = u0 - 0.5
            us = 0.5 - np.abs(U)
            arg = (2.0 * a / us + b) * U + m + 0.43
            k = np.floor(arg)
            mg = np.minimum(mg, np.minimum(arg - k, k + 1.0 - arg))
            fast_a, fast_b = us >= 0.07, V <= vr
            fast = fast_a & fast_b
            mg = np.minimum(mg, np.abs(us - 0.07))
            mg = np.where(fast_a, np.minimum(mg, np.abs(V - vr)), mg)
            rej_a = us < 0.013
            rej = (k < 0.0) | (rej_a & (V > us))
            slow = ~fast
            mg = np.where(slow, np.minimum(mg, np.abs(us - 0.013)), mg)
            mg = np.where(slow & rej_a, np.minimum(mg, np.abs(V - us)), mg)
            with np.errstate(invalid="ignore", divide="ignore"):
                lhs = np.log(V) + np.log(inv_alpha) - np.log(a / (us * us) + b)
                rhs = -m + k * np.log(m) - gammaln(k + 1.0)
            test = slow & ~rej
            mg = np.where(test, np.minimum(mg, np.abs(lhs - rhs)), mg)
            acc = fast | (test & (lhs <= rhs))
            idx = np.flatnonzero(todo)
            mb[idx] = mg
            ob[idx[acc]] = k[acc]
            todo[idx[acc]] = False
        out[big] = ob
        margin[big] = mb
    return out, margin


def draw(dist, a1, a2, a3, adr):
    """-> (values, margin): margin = +inf for the continuous families"""
    a1, a2, a3 = (np.broadcast_to(np.asarray(a, dtype="float64"), adr.shape) for a in (a1, a2, a3))
    inf = np.full(adr.shape, np.inf)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if dist == D_NORMAL:
            return np.where(a2 > 0, a1 + a2 * adr.normal(0), np.nan), inf
        if dist == D_HALFNORMAL:
            return np.where(a1 > 0, a1 * np.abs(adr.normal(0)), np.nan), inf
        if dist == D_LOGNORMAL:
            return np.where(a2 > 0, np.exp(a1 + a2 * adr.normal(0)), np.nan), inf
        u = adr.block(0)[0]
        if dist == D_CAUCHY:
            return np.where(a2 > 0, a1 + a2 * np.tan(np.pi * (u - 0.5)), np.nan), inf
        if dist == D_HALFCAUCHY:
            return np.where(a1 > 0, a1 * np.tan(0.5 * np.pi * u), np.nan), inf
        if dist == D_LAPLACE:
            v = np.where(u < 0.5, a1 + a2 * np.log(2.0 * u), a1 - a2 * np.log(2.0 * (1.0 - u)))
            return np.where(a2 > 0, v, np.nan), inf
        if dist == D_EXPONENTIAL:
            return np.where(a1 > 0, -np.log(u) / a1, np.nan), inf
        if dist == D_UNIFORM:
            return np.where(a1 <= a2, a1 + (a2 - a1) * u, np.nan), inf
        if dist == D_BERNOULLI:
            ok = (a1 >= 0) & (a1 <= 1)
            return np.where(ok, (u < a1).astype("float64"), np.nan), np.where(ok, np.abs(u - a1), np.inf)
        if dist == D_BERNOULLI_LOGIT:
            p = expit(a1)
            ok = ~np.isnan(a1)
            return np.where(ok, (u < p).astype("float64"), np.nan), np.where(ok, np.abs(u - p), np.inf)
        if dist == D_GAMMA:
            be = 1.0 / (1.0 / a2)
            ok = (a1 > 0) & (be > 0)
            return np.where(ok, gamma(np.where(ok, a1, 1.0), adr, 0) / be, np.nan), inf
        if dist == D_INVGAMMA:
            ok = (a1 > 0) & (a2 > 0)
            return np.where(ok, a2 / gamma(np.where(ok, a1, 1.0), adr, 0), np.nan), inf
        if dist == D_BETA:
            ok = (a1 > 0) & (a2 > 0)
            g1, g2 = gamma(np.where(ok, a1, 1.0), adr, 0), gamma(np.where(ok, a2, 1.0), adr, 2 * GAMMA_TRIES)
            return np.where(ok, g1 / (g1 + g2), np.nan), inf
        if dist == D_STUDENTT:
            ok = (a1 > 0) & (a3 > 0)
            nu = np.where(ok, a1, 1.0)
            g = gamma(0.5 * nu, adr, 0)
            return np.where(ok, a2 + a3 * adr.normal(T_BLOCK) / np.sqrt(2.0 * g / nu), np.nan), inf
        if dist == D_POISSON:
            ok = a1 >= 0
            k, mg = poisson(np.where(ok, a1, 1.0), adr)
            return np.where(ok, k, np.nan), np.where(ok, mg, np.inf)
    raise ValueError(f"family {dist} is refused")


def mixture(mu, sigma, w, adr):
    """mu, sigma, w: [..., K] broadcastable against adr.shape + (K,) -> (values, margin of the component pick)"""
    u = adr.block(0)[0]
    z = adr.normal(1)
    cw = np.cumsum(np.broadcast_to(w, adr.shape + (np.shape(w)[-1],)), axis=-1)
    K = cw.shape[-1]
    k = np.minimum((~(u[..., None] < cw)).sum(axis=-1), K - 1)
    margin = np.abs(u[..., None] - cw[..., : K - 1]).min(axis=-1) if K > 1 else np.full(adr.shape, np.inf)
    mu_k = np.take_along_axis(np.broadcast_to(mu, cw.shape), k[..., None], axis=-1)[..., 0]
    sg_k = np.take_along_axis(np.broadcast_to(sigma, cw.shape), k[..., None], axis=-1)[..., 0]
    return mu_k + sg_k * z, margin
