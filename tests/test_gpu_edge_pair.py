"""Edge pairing (option NUTS_EDGE_PAIR): a row pass that streams X for a tree leaf also evaluates the next leapfrog
of the trajectory's other end, and that leaf's later launch starts from the parked wave sums instead of streaming.

Every number the tree sees is formed by the code of the plain schedule from the plain schedule's operands, in tree order, so draws
and every numeric sampler statistic must be BITWISE those of NUTS_EDGE_PAIR=0 on the same seeds.

Shapes (group-aligned pass forced, NUTS_ROWS_GA=2; D = 8 with the intercept column): G = 40 and 65 (two blocks of records, the
last one ragged), 130 rows per group (two tiles: one wave without a tile, the last tile padded) and 300 (three tiles), packed
tiles and NUTS_GA_PACK=0.  Each run is made once per schedule and shared by the tests that look at it.

That the seeds exercise what is compared is asserted from the engine's own record (model scalars): shadow leaves were evaluated
and replayed, and some tree of depth >= 4 changed direction at least twice between its doublings."""

import functools

import numpy as np
import pytest

from pymc_amd import models

pytestmark = pytest.mark.gpu

TIMING = ("perf_counter_diff", "perf_counter_start", "process_time_diff")
SCALARS = ("edge_pair", "edge_pair_shadows", "edge_pair_replays", "edge_pair_turns", "edge_pair_ring_full", "edge_pair_dropped")
SHAPES = [(40, 130), (65, 130), (40, 300), (65, 300)]
CASES = [(G, R, pack) for (G, R) in SHAPES for pack in (1, 0)]

# what each kind of run asks of `sample` (the seed is part of the case: both schedules see the same streams)
RUNS = {
    # post-tuning draws in batches (nuts_chain_draw_many), after a tuning phase that adapts the step size
    "many": dict(tune=30, draws=40, seed=11, batch="64", kw={}),
    # every draw through nuts_chain_draw, tuning draws included
    "single": dict(tune=40, draws=4, seed=12, batch="1", kw={}),
    # a low energy limit: divergent draws (the tree stops inside a doubling, whatever was evaluated ahead is dropped)
    "divergent": dict(tune=30, draws=30, seed=13, batch="64", kw={"Emax": 1.0}),
    # a small fixed step under a depth limit of 8: every tree runs into the limit, and a 64-leaf doubling fills the ring
    "deep": dict(tune=0, draws=12, seed=14, batch="64", kw={"max_treedepth": 8, "early_max_treedepth": 8, "step_scale": 0.004}),
}


@functools.lru_cache(maxsize=None)
def _spec(G, R):
    return models.hier_logit(G=G, D=8, rows_per_group=R)


_cache = {}


def _run(monkeypatch, G, R, pack, kind, pair):
    key = (G, R, pack, kind, pair)
    if key in _cache:
        return _cache[key]
    from pymc_amd.sampling import sample

    r = RUNS[kind]
    monkeypatch.setenv("NUTS_ROWS_GA", "2")
    monkeypatch.setenv("NUTS_GA_PACK", str(pack))
    monkeypatch.setenv("NUTS_EDGE_PAIR", str(pair))
    monkeypatch.setenv("PYMC_AMD_DRAW_BATCH", r["batch"])
    res = sample(draws=r["draws"], tune=r["tune"], chains=1, model=_spec(G, R), init="adapt_diag", random_seed=r["seed"], device=0,
                 discard_tuned_samples=False, **r["kw"])
    f = res["step"]._logp_dlogp_func
    out = dict(draws=np.array(res["draws"]), stats=list(res["stats"][0]), warm=[],   # (`stats` holds the tuning draws too: nothing is discarded)
               scalars={k: f.model_scalar(k) for k in SCALARS},
               ga=f.model_scalar("rows_group_aligned"), packed=f.model_scalar("rows_packed"))
    res["step"].close()
    _cache[key] = out
    return out


def _same(a, b, what):
    assert np.array_equal(a["draws"], b["draws"]), what
    for name in ("warm", "stats"):
        assert len(a[name]) == len(b[name]), (what, name)
        for i, (x, y) in enumerate(zip(a[name], b[name])):
            assert set(x) == set(y)
            for key in x:
                if key in TIMING:
                    continue
                if key == "warning":
                    assert str(x[key]) == str(y[key]), (what, name, i)
                    continue
                xv, yv = np.asarray(x[key]), np.asarray(y[key])
                assert np.array_equal(xv, yv, equal_nan=xv.dtype.kind == "f"), (what, name, i, key, x[key], y[key])


def _pair_of_runs(monkeypatch, G, R, pack, kind):
    off = _run(monkeypatch, G, R, pack, kind, 0)
    on = _run(monkeypatch, G, R, pack, kind, 1)
    assert on["ga"] == 1.0 and on["packed"] == float(pack), (on["ga"], on["packed"])
    s, s0 = on["scalars"], off["scalars"]
    assert s0["edge_pair"] == 0.0 and s0["edge_pair_shadows"] == 0.0 and s0["edge_pair_replays"] == 0.0, s0
    print(f"G={G} R={R} pack={pack} {kind}: {s}")
    assert s["edge_pair"] == 1.0 and s["edge_pair_shadows"] > 0 and s["edge_pair_replays"] > 0, s
    return off, on


def _all(run):
    return run["warm"] + run["stats"]


@pytest.mark.parametrize("G,R,pack", CASES)
def test_tuned_draws_in_batches(G, R, pack, monkeypatch):
    off, on = _pair_of_runs(monkeypatch, G, R, pack, "many")
    assert max(int(s["depth"]) for s in _all(on)) >= 4 and on["scalars"]["edge_pair_turns"] >= 2, on["scalars"]
    _same(off, on, (G, R, pack))


@pytest.mark.parametrize("G,R,pack", CASES)
def test_tuning_draws_one_by_one(G, R, pack, monkeypatch):
    off, on = _pair_of_runs(monkeypatch, G, R, pack, "single")
    assert max(int(s["depth"]) for s in _all(on)) >= 4 and on["scalars"]["edge_pair_turns"] >= 2, on["scalars"]
    _same(off, on, (G, R, pack))


@pytest.mark.parametrize("G,R,pack", CASES)
def test_a_tree_shorter_than_the_one_before_drops_what_was_evaluated_ahead(G, R, pack, monkeypatch):
    """The look-ahead -- and with it the pairing -- goes as deep as the previous tree went: a tree that stops earlier leaves shadow
    leaves no tree uses (the engine counts them: still parked when their tree ended, or replayed only by a look-ahead doubling
    queued behind the tree's end), and the next tree starts from an empty ring."""
    off, on = _pair_of_runs(monkeypatch, G, R, pack, "many")
    depth = [int(s["depth"]) for s in _all(on)]
    assert any(b < a for a, b in zip(depth, depth[1:])), depth
    assert on["scalars"]["edge_pair_dropped"] > 0, on["scalars"]
    _same(off, on, (G, R, pack))


@pytest.mark.parametrize("G,R,pack", CASES)
def test_divergent_draws(G, R, pack, monkeypatch):
    off, on = _pair_of_runs(monkeypatch, G, R, pack, "divergent")
    div = [bool(s["diverging"]) for s in _all(on)]
    assert any(div) and not all(div), div
    _same(off, on, (G, R, pack))


@pytest.mark.parametrize("G,R,pack", CASES)
def test_depth_limit_and_full_ring(G, R, pack, monkeypatch):
    off, on = _pair_of_runs(monkeypatch, G, R, pack, "deep")
    assert any(bool(s["reached_max_treedepth"]) for s in _all(on))
    assert on["scalars"]["edge_pair_ring_full"] > 0, on["scalars"]
    _same(off, on, (G, R, pack))
