"""The edge-pairing launch with its two leaves side by side: `k_rows_ga_multi<2, 4, DX, true, PK>` evaluates row 0
of a lane under both coefficient vectors (`gam_row_pair<0>`, logit_row2 on {eta of the chain's leaf, eta of the shadow leaf}),
requests the wave's next tile, then row 1 (csrc/rows_ga_multi_kernel.h).  Per (leaf, row) the operations and their order are those
of the plain launch, so draws and every numeric sampler statistic must be BITWISE those of NUTS_EDGE_PAIR=0 on the same seed, on
packed and on raw tiles.

What the new loop can get wrong, and the shapes that show it (G = 12, D = 8, group-aligned pass forced with NUTS_ROWS_GA=2, four
waves per workgroup unless NUTS_ROWS_GA_W says otherwise; a lane holds rows 2l and 2l + 1 of a tile of 128):
  * the mask is now taken per row and applied to both leaves: 129 and 257 rows per group end in a tile of ONE row (lane 0: row 0
    valid, row 1 padded), 255 in a tile of 127 (lane 63: row 0 valid, row 1 padded);
  * the request sits between the two rows: with 129 / 257 rows every chunk is one tile, so the request made inside the loop is the
    re-read of the wave's last tile while row 1 is still to be evaluated from the decoded copy (NUTS_ROWS_GA_W=3 on 257 rows: three
    waves, one tile each, no wave without a tile); with 1500 rows the chunks are three tiles (first, middle, last);
  * row 1 is evaluated from `xx` after the tile registers were given to the request: values outside the exponent window (patched
    into `xx` on packed tiles) stand in rows 2k AND 2k + 1 of one lane, in a tile that is first and last of its chunk and in one
    that is neither, and in the last valid row next to a padded one;
  * the instantiation with eight stored columns (first column not all ones: `<2, 4, 8, true>`, raw tiles only) requests behind
    row 1;
  * a ring of two entries (NUTS_EDGE_PAIR_RING=2): shadow leaves are parked and replayed at the shortest distance.

That every shape keeps its packed copy (at most 1e-3 of the stored values outside the window, csrc/rows_pack.h) is checked on the
CPU from the data alone; on the device the engine's own record says which format the paired launch streamed."""

import numpy as np
import pytest

from pymc_amd.model_spec import ModelBuilder

TIMING = ("perf_counter_diff", "perf_counter_start", "process_time_diff")
SCALARS = ("edge_pair", "edge_pair_shadows", "edge_pair_replays", "edge_pair_turns", "edge_pair_packed", "edge_pair_rounds")
SCHED_VARS = ("NUTS_ROWS_GA", "NUTS_ROWS_GB", "NUTS_GA_AUX", "NUTS_ROWS_GA_W", "NUTS_FOLD_CTL", "NUTS_LEAN_STRICT", "NUTS_GA_PACK", "NUTS_GA_ONES0",
              "NUTS_EDGE_PAIR", "NUTS_EDGE_PAIR_RING")
G = 12
# `data`: rows per group, `ones0`: first column all ones (seven stored columns), `special`: {group: rows of the group} whose first
# and last stored column get a value outside the window.  Rows come in pairs (2k, 2k + 1) of one lane, or alone next to padding.
DATA = {
    # tiles 0 | 1 (one row): every chunk one tile.  Lane 5 of tile 0; the only row of the last tile
    "d129": dict(rows=129, ones0=True, special={0: [10, 11], 11: [128]}),
    # tiles 0 | 1 (127 rows).  Lane 0 of tile 0; lane 62 and lane 63 (row 0 only) of the last tile
    "d255": dict(rows=255, ones0=True, special={0: [0, 1], 5: [252, 253, 254], 11: [254]}),
    # tiles 0 | 1 | 2 (one row).  Lane 7 of tile 1 (first and last of its chunk), lane 63 of tile 0, the only row of the last tile
    "d257": dict(rows=257, ones0=True, special={0: [142, 143], 6: [126, 127], 11: [256]}),
    # twelve tiles, chunks of three.  Tile 4 (neither first nor last of its chunk: lane 9), tile 3 (first: lane 0), tile 11 (last of
    # the group, 92 rows: its last lane, 45), tile 5 / 6 across a chunk edge (lane 63 / lane 0)
    "d1500": dict(rows=1500, ones0=True, special={0: [530, 531], 3: [384, 385], 7: [1498, 1499], 11: [766, 767, 768, 769]}),
    # eight stored columns
    "d257x8": dict(rows=257, ones0=False, special={0: [142, 143], 11: [256]}),
}
CASES = {
    "r129": dict(data="d129", env={}, seed=11),
    "r255": dict(data="d255", env={}, seed=11),
    "r257": dict(data="d257", env={}, seed=11),
    "r257_w3": dict(data="d257", env={"NUTS_ROWS_GA_W": "3"}, seed=11),
    "r1500": dict(data="d1500", env={}, seed=11),
    "r1500_ring2": dict(data="d1500", env={"NUTS_EDGE_PAIR_RING": "2"}, seed=11),
    "r257x8": dict(data="d257x8", env={}, seed=11),
}
PACKED_AND_RAW = ["r129", "r255", "r257", "r257_w3", "r1500"]
OUTSIDE = [0.0, -1000.0, 5e-324, 2049.5, -(2.0 ** -30), 65536.0, 1e-300, -0.0]   # +-0, a denormal, tiny, far below and far beyond any window N(0, 1) data choose
RP_WINDOW, RP_MAX_EXC_SHARE = 16, 1e-3   # csrc/rows_pack.h
_data = {}
_specs = {}
_runs = {}


def _xy(name):
    if name in _data:
        return _data[name]
    d = DATA[name]
    sizes = np.full(G, d["rows"])
    rng = np.random.default_rng(21)
    N, D = int(sizes.sum()), 8
    gidx = np.repeat(np.arange(G), sizes).astype("int32")
    X = rng.normal(size=(N, D))
    if d["ones0"]:
        X[:, 0] = 1.0
    start = np.concatenate([[0], np.cumsum(sizes)])
    k = 0
    for g, rows in d["special"].items():
        for r in rows:
            for c in (1, 7):
                X[start[g] + r, c] = OUTSIDE[k % len(OUTSIDE)]
                k += 1
    beta = rng.normal(size=D) * 0.5
    with np.errstate(over="ignore"):
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-np.clip(X @ beta, -30, 30)))).astype("int8")
    _data[name] = (X, y, gidx)
    return _data[name]


def _outside_share(X):
    """rp_plan of csrc/rows_pack.h: share of the stored values (columns 1 .. 7) outside the best window of 16 binades"""
    e = ((X[:, 1:].astype("float64").view("uint64") >> np.uint64(52)) & np.uint64(0x7FF)).astype("int64").reshape(-1)
    hist = np.bincount(e, minlength=2048)
    inside = max(int(hist[lo:lo + RP_WINDOW].sum()) for lo in range(1, 2047 - RP_WINDOW + 1))
    return (e.size - inside) / e.size


@pytest.mark.parametrize("name", [n for n in DATA if DATA[n]["ones0"]])
def test_shapes_keep_their_packed_copy(name):
    X, y, _ = _xy(name)
    d = DATA[name]
    share = _outside_share(X)
    placed = 2 * sum(len(r) for r in d["special"].values())
    print(f"{name}: {share * X[:, 1:].size:.0f} of {X[:, 1:].size} stored values outside the window, {placed} of them placed")
    assert set(np.unique(y)) <= {0, 1} and np.all(X[:, 0] == 1.0)
    assert share <= RP_MAX_EXC_SHARE, share
    assert share * X[:, 1:].size >= placed   # (the placed values ARE outside the window the data choose)
    for rows in d["special"].values():       # pairs share a lane; a single row is the last valid row, its neighbour is padding
        odd = [r for r in rows if r % 2 == 0 and r + 1 not in rows]
        assert all(r == d["rows"] - 1 for r in odd), (name, odd)


def _spec(name):
    if name in _specs:
        return _specs[name]
    X, y, gidx = _xy(name)
    m = ModelBuilder()
    mu = m.Normal("mu", 0.0, 1.0, shape=8)
    sigma = m.HalfNormal("sigma", 1.0, shape=8)
    z = m.Normal("z", 0.0, 1.0, shape=(G, 8))
    m.HierLogitRows("y", X, y, gidx, mu, sigma, z)
    _specs[name] = m.build()
    return _specs[name]


def _run(monkeypatch, case, pack, pair):
    env = dict(CASES[case]["env"])
    if not pair:
        env.pop("NUTS_EDGE_PAIR_RING", None)   # (no ring without pairing: the same reference run serves both)
    key = (CASES[case]["data"], tuple(sorted(env.items())), CASES[case]["seed"], pack, pair)
    if key in _runs:
        return _runs[key]
    from pymc_amd.sampling import sample

    for k in SCHED_VARS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NUTS_ROWS_GA", "2")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("NUTS_GA_PACK", str(pack))
    monkeypatch.setenv("NUTS_EDGE_PAIR", str(pair))
    res = sample(draws=40, tune=30, chains=1, model=_spec(CASES[case]["data"]), init="adapt_diag", random_seed=CASES[case]["seed"], device=0,
                 discard_tuned_samples=False)
    f = res["step"]._logp_dlogp_func
    out = dict(draws=np.array(res["draws"]), stats=list(res["stats"][0]), scalars={k: f.model_scalar(k) for k in SCALARS},
               ga=f.model_scalar("rows_group_aligned"), packed=f.model_scalar("rows_packed"), waves=f.model_scalar("rows_waves"))
    res["step"].close()
    _runs[key] = out
    return out


def _check(monkeypatch, case, pack, packed_expected):
    off = _run(monkeypatch, case, pack, 0)
    on = _run(monkeypatch, case, pack, 1)
    s, s0 = on["scalars"], off["scalars"]
    depth = [int(x["depth"]) for x in on["stats"]]
    print(f"{case} pack={pack}: {s}; waves {on['waves']}; max depth {max(depth)}")
    assert on["ga"] == 1.0 and on["packed"] == float(packed_expected), (on["ga"], on["packed"])
    assert on["waves"] == float(CASES[case]["env"].get("NUTS_ROWS_GA_W", 4)), on["waves"]
    assert s0["edge_pair"] == 0.0 and s0["edge_pair_shadows"] == 0.0 and s0["edge_pair_replays"] == 0.0, s0
    assert s["edge_pair"] == 1.0 and s["edge_pair_shadows"] > 0 and s["edge_pair_replays"] > 0 and s["edge_pair_turns"] >= 2, s
    assert s["edge_pair_packed"] == float(packed_expected) and s["edge_pair_rounds"] == 1.0, s
    assert len(on["stats"]) == len(off["stats"]) == 70
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


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [1, 0])
@pytest.mark.parametrize("case", PACKED_AND_RAW)
def test_side_by_side_bitwise_against_pairing_off(case, pack, monkeypatch):
    _check(monkeypatch, case, pack, pack)


@pytest.mark.gpu
def test_eight_stored_columns_bitwise_against_pairing_off(monkeypatch):
    # (a first column that is not all ones is stored: no packed copy, whatever NUTS_GA_PACK says)
    _check(monkeypatch, "r257x8", 1, 0)


@pytest.mark.gpu
def test_ring_of_two_bitwise_against_pairing_off(monkeypatch):
    _check(monkeypatch, "r1500_ring2", 1, 1)
