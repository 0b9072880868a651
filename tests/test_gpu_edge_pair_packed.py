"""The edge-pairing launch on the tiles the chain's own launch streams, every workgroup resident at once:
`k_rows_ga_multi<2, 4, 7, true, 1>` on packed tiles, `k_rows_ga_multi<2, 4, 7, true>` on raw ones (csrc/rows_ga_multi_kernel.h).

The shadow leaf is evaluated on a tile decoded and patched inside the paired launch and parked in the ring; a wrong patch, decode
or tile address changes a ring entry and thereby the bits of a later leaf, so draws and every numeric sampler statistic must be
BITWISE those of NUTS_EDGE_PAIR=0 on the same seed, under both tile formats.

Models as tests/test_gpu_rows_packed.py builds them (G = 12, D = 8, intercept column of ones, group-aligned pass forced with
NUTS_ROWS_GA=2), with values outside the exponent window in the first and last tile of a chunk and next to a group's padded rows.
Shapes: 130 rows per group (waves without a tile: the slack tile is read; a last tile of 2 rows), 901 rows with three waves (chunks
of 2 / 3 / 3 tiles: odd counts, both halves, both streaming orders), 2500 rows (uniform geometry, five tiles per wave: the request
made inside the loop is consumed), ragged groups of 130 / 300 / 901 rows (chunk offsets and exception index from the tables).

That the seeds exercise what is compared is asserted from the engine's own record (model scalars): shadow leaves were evaluated and
replayed, some tree of depth >= 4 changed direction at least twice, the paired launch streamed the format asked for, and its grid
fits one round."""

import numpy as np
import pytest

from pymc_amd.model_spec import ModelBuilder

pytestmark = pytest.mark.gpu

TIMING = ("perf_counter_diff", "perf_counter_start", "process_time_diff")
SCALARS = ("edge_pair", "edge_pair_shadows", "edge_pair_replays", "edge_pair_turns", "edge_pair_packed", "edge_pair_rounds")
SCHED_VARS = ("NUTS_ROWS_GA", "NUTS_ROWS_GB", "NUTS_GA_AUX", "NUTS_ROWS_GA_W", "NUTS_FOLD_CTL", "NUTS_LEAN_STRICT", "NUTS_GA_PACK", "NUTS_GA_ONES0",
              "NUTS_EDGE_PAIR", "NUTS_EDGE_PAIR_RING")
G = 12
# `special`: {group: rows of the group} that get values outside the window in their first and last stored column; an eligible model
# holds at most 1e-3 of its values outside the window, which bounds how many a shape takes (positions of tests/test_gpu_rows_packed.py)
SHAPES = {
    "r130": dict(sizes=[130] * G, env={}, seed=11, special={0: [0, 127, 129], 11: [128]}),
    "r901_w3": dict(sizes=[901] * G, env={"NUTS_ROWS_GA_W": "3"}, seed=11, special={g: [0, 255, 256, 639, 640, 896, 899, 900] for g in (0, 5, 11)}),
    "r2500": dict(sizes=[2500] * G, env={}, seed=11, special={g: [0, 127, 128, 639, 640, 1279, 1280, 2432, 2498, 2499] for g in (0, 7, 11)}),
    "ragged": dict(sizes=[130, 300, 901, 901, 130, 300, 300, 901, 130, 130, 901, 300], env={}, seed=11,
                   special={0: [0, 129], 1: [0, 128, 256, 299], 2: [0, 255, 256, 768, 900]}),
}
OUTSIDE = [0.0, -0.0, 5e-324, 1e-300, -(2.0 ** -14), 8.0, -17.0, 20.25]   # +-0, a denormal, tiny, just below, just above, beyond
EDGES = [2.0 ** -13, -(2.0 ** -12), np.nextafter(8.0, 0.0), -np.nextafter(16.0, 0.0), 2.0 ** -12, 16.0]   # first / last values of a window, and past them
_specs = {}
_runs = {}


def _spec(shape):
    if shape in _specs:
        return _specs[shape]
    sizes = np.asarray(SHAPES[shape]["sizes"])
    rng = np.random.default_rng(21)
    N, D = int(sizes.sum()), 8
    gidx = np.repeat(np.arange(G), sizes).astype("int32")
    X = rng.normal(size=(N, D))
    X[:, 0] = 1.0
    start = np.concatenate([[0], np.cumsum(sizes)])
    k = 0
    for g, rows in SHAPES[shape]["special"].items():
        for r in rows:
            for c in (1, 7):
                X[start[g] + r, c] = OUTSIDE[k % len(OUTSIDE)]
                k += 1
            X[start[g] + r, 2 + k % 5] = EDGES[k % len(EDGES)]
    beta = rng.normal(size=D) * 0.5
    with np.errstate(over="ignore"):
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-np.clip(X @ beta, -30, 30)))).astype("int8")
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0, shape=D)
    sigma = m.HalfNormal("sigma", 1.0, shape=D)
    z = m.Normal("z", 0.0, 1.0, shape=(G, D))
    m.HierLogitRows("y", X, y, gidx, mu, sigma, z)
    _specs[shape] = m.build()
    return _specs[shape]


def _run(monkeypatch, shape, pack, pair):
    key = (shape, pack, pair)
    if key in _runs:
        return _runs[key]
    from pymc_amd.sampling import sample

    for k in SCHED_VARS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NUTS_ROWS_GA", "2")
    for k, v in SHAPES[shape]["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("NUTS_GA_PACK", str(pack))
    monkeypatch.setenv("NUTS_EDGE_PAIR", str(pair))
    res = sample(draws=40, tune=30, chains=1, model=_spec(shape), init="adapt_diag", random_seed=SHAPES[shape]["seed"], device=0,
                 discard_tuned_samples=False)
    f = res["step"]._logp_dlogp_func
    out = dict(draws=np.array(res["draws"]), stats=list(res["stats"][0]), scalars={k: f.model_scalar(k) for k in SCALARS},
               ga=f.model_scalar("rows_group_aligned"), packed=f.model_scalar("rows_packed"))
    res["step"].close()
    _runs[key] = out
    return out


@pytest.mark.parametrize("pack", [1, 0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_paired_launch_bitwise_against_pairing_off(shape, pack, monkeypatch):
    off = _run(monkeypatch, shape, pack, 0)
    on = _run(monkeypatch, shape, pack, 1)
    s, s0 = on["scalars"], off["scalars"]
    depth = [int(x["depth"]) for x in on["stats"]]
    print(f"{shape} pack={pack}: {s}; max depth {max(depth)}")
    assert on["ga"] == 1.0 and on["packed"] == float(pack), (on["ga"], on["packed"])
    assert s0["edge_pair"] == 0.0 and s0["edge_pair_shadows"] == 0.0 and s0["edge_pair_replays"] == 0.0, s0
    assert s["edge_pair"] == 1.0 and s["edge_pair_shadows"] > 0 and s["edge_pair_replays"] > 0 and s["edge_pair_turns"] >= 2, s
    assert s["edge_pair_packed"] == float(pack) and s["edge_pair_rounds"] == 1.0, s
    assert len(on["stats"]) == len(off["stats"]) == 70 and max(depth) >= 4, depth
    assert np.array_equal(on["draws"], off["draws"])
    for i, (x, y) in enumerate(zip(on["stats"], off["stats"])):
        assert set(x) == set(y)
        for key in x:
            if key in TIMING:
                continue
            if key == "warning":
                assert str(x[key]) == str(y[key]), i
                continue
            xv, yv = np.asarray(x[key]), np.asarray(y[key])
            assert np.array_equal(xv, yv, equal_nan=xv.dtype.kind == "f"), (i, key, x[key], y[key])
