"""The group-aligned row pass on packed tiles (csrc/rows_pack.h, `k_rows_ga<8, 2, 7, 1>`) against the same model on raw tiles.

The packing is lossless and the kernel hands `ga_tile` the operands the raw tile would have given it, so nothing may differ:
logp / gradient BITWISE at three points under both streaming orders (`rev` alternates from launch to launch), and a short NUTS
chain bitwise, draws and integer statistics.  `NUTS_GA_PACK=0` keeps the raw tiles; `NUTS_ROWS_GA=2` forces the group-aligned pass
on these small shapes, as tests/test_gpu_rows_generalised.py does.

Shapes: 130 rows per group (two tiles over four waves: waves without a tile, a last tile of 2 rows), 901 rows per group with three
waves (eight tiles in chunks of 2 / 3 / 3: odd counts, both halves), 2500 rows per group (twenty tiles, five per wave, uniform
geometry: the shape class of the benchmark), ragged groups of 130 / 300 / 901 rows (chunk offsets from the table).

Values outside the exponent window sit in the first and the last tile of a chunk and next to the masked padding rows of a group's
last tile: +-0, a denormal, tiny and large magnitudes, and the window's edges in every shape; +-1e300 (an exponent far from any
window) in a shape of its own, `r130_far`, which is compared on logp / gradient only -- a covariate of 1e300 gives gradients of
1e300, every leapfrog step diverges and a chain shows nothing.  NaN and inf are NOT injected on the GPU: one such covariate makes
logp and every gradient element of its group NaN under both layouts, and a comparison of NaN with NaN would pass whatever the
patch did (the tests assert finite results).  They take the same path as +-1e300 through the kernel (biased exponent outside the
window -> raw bits from the exception list), and the packer's side of them is checked bit for bit on the CPU
(tests/test_rows_pack_cpu.py).
"""

import numpy as np
import pytest

from pymc_amd.model_spec import ModelBuilder

pytestmark = pytest.mark.gpu

INT_KEYS = ("depth", "tree_size", "index_in_trajectory", "diverging", "reached_max_treedepth")
SCHED_VARS = ("NUTS_ROWS_GA", "NUTS_ROWS_GB", "NUTS_GA_AUX", "NUTS_ROWS_GA_W", "NUTS_FOLD_CTL", "NUTS_LEAN_STRICT", "NUTS_GA_PACK", "NUTS_GA_ONES0")
G = 12
# `special`: {group: rows of the group} that get values outside the window in their first and last stored column (slots 0 / 1 and
# 12 / 13 of a lane).  An eligible model may hold at most 1e-3 of its values outside the window, which bounds how many a shape takes.
SHAPES = {
    # two tiles over four waves (tiles with waves 1 and 3): first / last lane of the first tile, the last tile's two valid rows
    "r130": dict(sizes=[130] * G, env={}, special={0: [0, 127, 129], 11: [128]}),
    # chunks [0, 2), [2, 5), [5, 8): first and last row of every chunk, the last tile's first and last valid rows
    "r901_w3": dict(sizes=[901] * G, env={"NUTS_ROWS_GA_W": "3"}, special={g: [0, 255, 256, 639, 640, 896, 899, 900] for g in (0, 5, 11)}),
    # uniform geometry (chunk offsets from the stride, no table), five tiles per wave: the tiles requested inside the streaming
    # loop are consumed (with three tiles or fewer per wave only the two requested ahead of the loop are)
    "r2500": dict(sizes=[2500] * G, env={}, special={g: [0, 127, 128, 639, 640, 1279, 1280, 2432, 2498, 2499] for g in (0, 7, 11)}),
    # r130's positions with +-1e300: logp / gradient only (see the module docstring)
    "r130_far": dict(sizes=[130] * G, env={}, special={0: [0, 127, 129], 11: [128]}, outside=[1e300, -1e300], chain=False),
    "ragged": dict(sizes=[130, 300, 901, 901, 130, 300, 300, 901, 130, 130, 901, 300], env={},
                   special={0: [0, 129], 1: [0, 128, 256, 299], 2: [0, 255, 256, 768, 900]}),
}
# (small samples may prefer the window [-12, 4) to the [-13, 3) of large ones: the lists straddle both)
OUTSIDE = [0.0, -0.0, 5e-324, 1e-300, -(2.0 ** -14), 8.0, -17.0, 20.25]   # +-0, a denormal, tiny, just below, just above, beyond
EDGES = [2.0 ** -13, -(2.0 ** -12), np.nextafter(8.0, 0.0), -np.nextafter(16.0, 0.0), 2.0 ** -12, 16.0]   # first / last values of a window, and past them
_cache = {}


def _spec(shape, dummy=False):
    key = (shape, dummy)
    if key in _cache:
        return _cache[key]
    sizes = np.asarray(SHAPES[shape]["sizes"])
    rng = np.random.default_rng(21)
    N, D = int(sizes.sum()), 8
    gidx = np.repeat(np.arange(G), sizes).astype("int32")
    X = rng.normal(size=(N, D))
    X[:, 0] = 1.0
    start = np.concatenate([[0], np.cumsum(sizes)])
    outside = SHAPES[shape].get("outside", OUTSIDE)
    k = 0
    for g, rows in SHAPES[shape]["special"].items():
        for r in rows:
            for c in (1, 7):
                X[start[g] + r, c] = outside[k % len(outside)]
                k += 1
            X[start[g] + r, 2 + k % 5] = EDGES[k % len(EDGES)]
    if dummy:
        X[:, 4] = (rng.random(N) < 0.5).astype("float64")
    beta = rng.normal(size=D) * 0.5
    with np.errstate(over="ignore"):
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-np.clip(X @ beta, -30, 30)))).astype("int8")
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0, shape=D)
    sigma = m.HalfNormal("sigma", 1.0, shape=D)
    z = m.Normal("z", 0.0, 1.0, shape=(G, D))
    m.HierLogitRows("y", X, y, gidx, mu, sigma, z)
    _cache[key] = m.build()
    return _cache[key]


def _env(monkeypatch, shape, pack):
    for k in SCHED_VARS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NUTS_ROWS_GA", "2")
    for k, v in SHAPES[shape]["env"].items():
        monkeypatch.setenv(k, v)
    if not pack:
        monkeypatch.setenv("NUTS_GA_PACK", "0")


def _values(spec, want_packed):
    """logp / gradient at three points, each evaluated twice: consecutive launches stream the halves in the other order."""
    from pymc_amd.value_grad import DeviceValueGradFunction

    f = DeviceValueGradFunction(spec, device=0)
    assert f.model_scalar("rows_group_aligned") == 1.0 and f.model_scalar("rows_group_block") == 0.0
    assert f.model_scalar("rows_packed") == want_packed
    rng = np.random.default_rng(3)
    out = []
    for q in [np.zeros(spec.n)] + [rng.normal(size=spec.n) * s for s in (0.3, 0.7)]:
        for _ in range(2):
            lp, g = f._pytensor_function(q)
            out.append((np.float64(lp).tobytes(), np.asarray(g, dtype="float64").tobytes()))
            assert np.isfinite(lp) and np.all(np.isfinite(g))
    f.close()
    return out


def _chain(spec):
    from pymc_amd.sampling import sample

    res = sample(draws=12, tune=8, chains=1, model=spec, init="adapt_diag", random_seed=17, device=0, discard_tuned_samples=False)
    stats = res["stats"][0]
    draws = np.asarray(res["draws"][0]).copy()
    res["step"].close()
    return draws, stats


@pytest.mark.parametrize("shape", list(SHAPES))
def test_packed_logp_grad_bitwise(shape, monkeypatch):
    spec = _spec(shape)
    _env(monkeypatch, shape, pack=True)
    packed = _values(spec, 1.0)
    _env(monkeypatch, shape, pack=False)
    raw = _values(spec, 0.0)
    assert packed == raw
    # the two streaming orders sum the same halves: the second evaluation of a point repeats the first
    assert all(packed[i] == packed[i + 1] for i in range(0, len(packed), 2))


@pytest.mark.parametrize("shape", [k for k, v in SHAPES.items() if v.get("chain", True)])
def test_packed_nuts_chain_bitwise(shape, monkeypatch):
    spec = _spec(shape)
    _env(monkeypatch, shape, pack=True)
    d1, s1 = _chain(spec)
    _env(monkeypatch, shape, pack=False)
    d0, s0 = _chain(spec)
    depths = [int(s["depth"]) for s in s1]
    print("tree depths:", depths)
    assert len(s1) == len(s0) == 20 and max(depths) >= 3
    assert d1.tobytes() == d0.tobytes()
    for a, b in zip(s1, s0):
        for k in INT_KEYS:
            assert int(a[k]) == int(b[k]), k


def test_dummy_column_keeps_the_raw_tiles(monkeypatch):
    """Half of a 0/1 column's values are zeros -- exceptions: far beyond the 1e-3 cap, so the model streams raw tiles."""
    spec = _spec("r130", dummy=True)
    _env(monkeypatch, "r130", pack=True)
    a = _values(spec, 0.0)
    _env(monkeypatch, "r130", pack=False)
    assert a == _values(spec, 0.0)
