"""Models, refusal cases and the conditional CDFs the prior-predictive tests share (tests/test_prior_host.py on the host,
tests/test_gpu_prior.py on the device)."""
import numpy as np
from scipy import stats

import prior_reference as pref
from pymc_amd import model_spec as ms
from pymc_amd import models
from pymc_amd.model_spec import ModelBuilder

BARE = lambda k: ms.Term(ms.Operand(ms.OP_VAR, 0.0, k))   # noqa: E731
CONST = lambda c: ms.Term(ms.Operand(ms.OP_CONST, float(c)))   # noqa: E731


def chain3(N=5):
    """three deep: s ~ HalfNormal, m ~ Normal(0, s), x[N] ~ Normal(m, exp(m) * s) -- the scale through a program"""
    m = ModelBuilder()
    s = m.HalfNormal("s", 1.0)
    mm = m.Normal("m", 0.0, s)
    m.Normal("x", mm, m.math.exp(mm) * s, shape=N)
    return m.build()


def gathered(N=7, A=7, seed=3):
    """a child whose mean gathers a parent: b[N] ~ Normal(a[idx], 1)"""
    idx = np.random.default_rng(seed).integers(0, A, size=N)
    idx[: min(A, N)] = np.arange(min(A, N))
    m = ModelBuilder()
    a = m.Normal("a", 0.0, 1.0, shape=A)
    m.Normal("b", a[idx], 1.0, shape=N)
    return m.build()


def every_family(N=250):
    """every continuous family the variates cover and every transform: log (HalfNormal, Gamma, ...), logodds (Beta), interval with
    the bounds -1 and 3 (Uniform), none; a scalar parent that broadcasts (s), element-wise vector parents (loc, sc, un, be, ex)"""
    m = ModelBuilder()
    s = m.HalfNormal("s", 1.3)
    loc = m.Normal("loc", 0.5, 2.0, shape=N)
    sc = m.Gamma("sc", 2.5, 2.0, shape=N)
    be = m.Beta("be", 0.7, 2.5, shape=N)
    un = m.Uniform("un", -1.0, 3.0, shape=N)
    ex = m.Exponential("ex", sc, shape=N)
    m.Normal("n1", loc, sc, shape=N)
    m.Cauchy("c1", loc, s, shape=N)
    m.HalfCauchy("hc", sc, shape=N)
    m.StudentT("t1", 4.0, loc, s, shape=N)
    m.LogNormal("ln", loc, 0.7, shape=N)
    m.InverseGamma("ig", 3.0, s, shape=N)
    m.Laplace("la", un, sc, shape=N)
    m.HalfNormal("hn", be, shape=N)
    m.Gamma("ga", 0.5, ex, shape=N)
    m.Normal("y", loc, 1.0, observed=np.linspace(-2.0, 2.0, N))
    return m.build()


def sized(size):
    """two levels over variables of `size` elements, each transform among them: the shapes at which the level kernel's workgroups end"""
    m = ModelBuilder()
    s = m.HalfNormal("s", 1.0, shape=size)
    p = m.Beta("p", 2.0, 3.0, shape=size)
    u = m.Uniform("u", -1.0, 3.0, shape=size)
    m.Normal("x", u, s, shape=size)
    m.Gamma("g", 1.5, p, shape=size)
    return m.build()


def dirichlet_mixture(K=3, N=40, alpha=None, seed=11):
    """the marginal Normal mixture with w ~ Dirichlet(alpha): the node owns the weights' prior"""
    rng = np.random.default_rng(seed)
    alpha = np.linspace(0.6, 2.4, K) if alpha is None else np.asarray(alpha, dtype="float64")
    m = ModelBuilder()
    w = m.Dirichlet("w", alpha)
    mu = m.Normal("mu", 0.0, 3.0, shape=K)
    sigma = m.HalfNormal("sigma", 2.0, shape=K)
    m.NormalMixture("y", w, mu, sigma, rng.normal(size=N) * 2.0)
    return m.build()


def nan_model(N=9):
    """x ~ Normal(0, m) with m ~ Normal(0, 1): invalid wherever m <= 0; z ~ Normal(x, 1) below it"""
    m = ModelBuilder()
    mm = m.Normal("m", 0.0, 1.0)
    x = m.Normal("x", 0.0, mm, shape=N)
    m.Normal("z", x, 1.0, shape=N)
    return m.build()


def with_deterministics(N=6):
    """a scalar and a vector Deterministic over transformed variables: what `prior` holds next to the variables"""
    m = ModelBuilder()
    s = m.HalfNormal("s", 1.0)
    x = m.Normal("x", 0.0, s, shape=N)
    m.Deterministic("s2", s * s)
    m.Deterministic("ex", m.math.exp(x) * s)
    m.Normal("y", x, 1.0, observed=np.linspace(-1.0, 1.0, N))
    return m.build()


# ---- refusals: (label, spec builder, text both layers must give, the engine can be asked) ------------------------------------------
def _flat():
    m = ModelBuilder()
    m.Normal("a", 0.0, 1.0)
    m.Flat("free", shape=3)
    return m.build()


def _twice():
    m = ModelBuilder()
    m.Normal("a", 0.0, 1.0)
    m.Normal("twice", 0.0, 1.0, shape=3)
    m.spec.factors.append(ms.Factor(ms.D_NORMAL, 3, (BARE(1), CONST(1.0), CONST(2.0)), 0.0, "twice_again"))
    return m.build()


def _weibull():
    """a prior lowered op by op: a Potential over a free value variable"""
    m = ModelBuilder()
    w = m.Flat("weib")
    m.Potential("weib_logp", m.math.log(m.math.exp(w)) - m.math.exp(w))
    return m.build()


def _truncated():
    m = ModelBuilder()
    m.TruncatedNormal("trunc", 0.0, 1.0, lower=-1.0, upper=2.0, shape=4)
    return m.build()


def _by_hand(dist, name, nargs):
    def build():
        m = ModelBuilder()
        m.Normal("a", 0.0, 1.0)
        m.Flat(name, shape=2)
        m.spec.factors.append(ms.Factor(dist, 2, (BARE(1),) + tuple(CONST(0.5) for _ in range(nargs - 1)), 0.0, name))
        return m.build()
    return build


def _lin_prior():
    X = np.random.default_rng(2).normal(size=(6, 3))
    m = ModelBuilder()
    beta = m.Normal("beta", 0.0, 1.0, shape=3)
    m.Normal("linchild", m.dot(X, beta), 1.0, shape=6)
    return m.build()


def _derived_prior():
    X = np.random.default_rng(2).normal(size=(6, 3))
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0)
    z = m.Normal("z", 0.0, 1.0, shape=3)
    m.Normal("derchild", m.dot(X, mu + 0.5 * z), 1.0, shape=6)
    return m.build()


def _many_variables():
    m = ModelBuilder()
    for k in range(0x4001):
        m.spec.vars.append(ms.FreeVar(f"v{k}", (2,), ms.TR_NONE, 0.0, 1.0, 2 * k))
        m.spec.factors.append(ms.Factor(ms.D_NORMAL, 2, (BARE(k), CONST(0.0), CONST(1.0)), 0.0, f"v{k}"))
    return m.build()


def _potential_reweights():
    m = ModelBuilder()
    a = m.Normal("pushed", 0.0, 1.0, shape=3)
    m.Potential("push", -(a * a))
    return m.build()


REFUSALS = [
    ("no factor", _flat, "variable 1 ('free') has no prior factor", True),
    ("two factors", _twice, "variable 1 ('twice') has more than one prior factor", True),
    ("lowered op by op", _weibull, "reads variable 0 ('weib'): it reweights the prior", True),
    ("TruncatedNormal", _truncated, "variable 0 ('trunc'): its prior is a TruncatedNormal factor", True),
    ("Binomial", _by_hand(ms.D_BINOMIAL, "binom", 4), "variable 1 ('binom'): its prior is a Binomial factor", True),
    ("Derived", _by_hand(ms.D_DERIVED, "deriv", 1), "variable 1 ('deriv'): its prior is a Derived factor", True),
    ("discrete", _by_hand(ms.D_POISSON, "pois", 3), "variable 1 ('pois'): its prior is a discrete Poisson factor", True),
    ("Potential reweights", _potential_reweights, "reads variable 0 ('pushed'): it reweights the prior", True),
    ("linear predictor", _lin_prior, "variable 1 ('linchild'): its prior reads a linear predictor or a derived vector", True),
    ("derived vector", _derived_prior, "variable 2 ('derchild'): its prior reads a linear predictor or a derived vector", True),
    ("MvNormal node", lambda: models.mvnormal(n=16, seed=5), "variable 0 ('x') is the MvNormal node's", True),
    ("conditional mixture", lambda: models.normal_mixture_bayes(N=40, K=3), "is a conditional mixture", True),
    # (a spec of 16 385 variables is more than the engine's other tables take: the host layer alone is asked)
    ("index above 16383", _many_variables, "variable 16384 ('v16384'): its index does not fit", False),
]


def engine_text(text):
    """the engine knows a variable by its place in the spec, not by its name"""
    import re

    return re.sub(r" \('[^']*'\)", "", text)


# ---- conditional CDFs ---------------------------------------------------------------------------------------------------------------
def cdf(dist, x, a1, a2, a3):
    with np.errstate(all="ignore"):
        if dist == ms.D_NORMAL:
            return stats.norm.cdf(x, a1, a2)
        if dist == ms.D_HALFNORMAL:
            return stats.halfnorm.cdf(x, scale=a1)
        if dist == ms.D_CAUCHY:
            return stats.cauchy.cdf(x, a1, a2)
        if dist == ms.D_HALFCAUCHY:
            return stats.halfcauchy.cdf(x, scale=a1)
        if dist == ms.D_STUDENTT:
            return stats.t.cdf(x, a1, a2, a3)
        if dist == ms.D_BETA:
            return stats.beta.cdf(x, a1, a2)
        if dist == ms.D_EXPONENTIAL:
            return stats.expon.cdf(x, scale=1.0 / a1)
        if dist == ms.D_UNIFORM:
            return stats.uniform.cdf(x, a1, a2 - a1)
        if dist == ms.D_LOGNORMAL:
            return stats.lognorm.cdf(x, a2, scale=np.exp(a1))
        if dist == ms.D_GAMMA:
            return stats.gamma.cdf(x, a1, scale=1.0 / a2)
        if dist == ms.D_INVGAMMA:
            return stats.invgamma.cdf(x, a1, scale=a2)
        if dist == ms.D_LAPLACE:
            return stats.laplace.cdf(x, a1, a2)
    raise ValueError(dist)


def conditional_u(spec, q):
    """{variable: F(x | the parents' drawn values) [S, size]} for every variable with a prior factor, from positions q [S, n]"""
    from pymc_amd import predictive

    x = pref.constrained(spec, q)
    by_name = {v.name: v for v in spec.vars}
    out = {}
    for level in predictive.prior_plan(spec):
        for name, fi in level:
            if fi < 0:
                continue
            v = by_name[name]
            a1, a2, a3 = pref.factor_args(spec, fi, x)
            out[name] = cdf(spec.factors[fi].dist, x[:, v.offset : v.offset + v.size], a1, a2, a3)
    return out


def sup_uniform(u):
    """sup |ECDF - u| of values that should be uniform on (0, 1)"""
    u = np.sort(np.ravel(u))
    n = u.size
    return float(max((np.arange(1, n + 1) / n - u).max(), (u - np.arange(n) / n).max()))


def parents_elementwise(spec):
    """(child, parent) pairs of equal size: the parent is read element by element (or both are scalars)"""
    from pymc_amd import predictive

    size = {v.name: v.size for v in spec.vars}
    pairs = []
    for level in predictive.prior_plan(spec):
        for name, fi in level:
            if fi < 0:
                continue
            for o in predictive._operands(spec.factors[fi], 1):
                if o.kind == ms.OP_VAR and size[spec.vars[o.ref].name] == size[name] and (name, spec.vars[o.ref].name) not in pairs:
                    pairs.append((name, spec.vars[o.ref].name))
    return pairs
