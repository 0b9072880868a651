"""The host-side plan of edge pairing (csrc/engine.hip `EdgePlan`, DESIGN.md 4.15, through `nuts_edge_pair_plan`) against a
brute-force enumeration: every direction sequence of up to seven doublings (depth <= 6 as the doublings are numbered), every
look-ahead depth, several ring sizes and depth limits.

The enumeration below states the rules from scratch and follows every launch: a leaf whose wave sums were evaluated ahead must be a
replay of exactly that entry; a streamed leaf takes the other end's next leapfrog with it exactly when that end's next doubling
is one the look-ahead knows and neither that doubling nor the ring is full; a shadow leaf is always the successor of the last one
evaluated for its end (so it never runs ahead of its source state), and no ring slot is written while it holds an entry that has
not been replayed."""

import ctypes as C
import itertools

import numpy as np

from pymc_amd import _lib

PLAIN, PAIRED, REPLAY = 0, 1, 2


def _plan(dirs, n_doublings, spec, max_depth, ring):
    lib = _lib.load()
    d = np.asarray(dirs, dtype=np.int32)
    out = np.zeros(5 * (1 << n_doublings), dtype=np.int32)
    n = lib.nuts_edge_pair_plan(d.ctypes.data_as(C.POINTER(C.c_int32)), len(d), n_doublings, spec, max_depth, ring,
                                out.ctypes.data_as(C.POINTER(C.c_int32)), len(out) // 5)
    assert n == (1 << n_doublings) - 1, (n, dirs)
    return out[: 5 * n].reshape(n, 5)


def _check(dirs, n_doublings, spec, max_depth, ring):
    plan = _plan(dirs, n_doublings, spec, max_depth, ring)
    last = min(spec, max_depth - 1, len(dirs) - 1)
    ahead = {1: [], -1: []}   # per end: ring slots of the leaves evaluated ahead and not yet replayed, leaf 0 first
    held = set()              # ring slots in use
    i = 0
    counts = [0, 0, 0]
    for d in range(n_doublings):
        D = dirs[d]
        mine = list(ahead[D])
        assert len(mine) <= 1 << d, (dirs, d)           # an end never holds more than its next doubling has leaves
        nxt = next((e for e in range(d + 1, last + 1) if dirs[e] == -D), None)
        for j in range(1 << d):
            dd, jj, kind, slot, k = (int(v) for v in plan[i])
            i += 1
            assert (dd, jj) == (d, j)
            counts[kind] += 1
            if j < len(mine):                             # evaluated ahead: the launch must skip the stream, from that entry
                assert kind == REPLAY and k == j and slot == mine[j], (dirs, d, j, plan[i - 1])
                held.discard(slot)
                ahead[D].pop(0)
                continue
            assert not ahead[D]                           # everything this end held has been consumed before its first streamed leaf
            other = ahead[-D]
            room = nxt is not None and len(other) < min(1 << nxt, ring) and len(held) < ring
            if room:
                # the successor of the last leaf evaluated for that end (its source state exists), into a free slot
                assert kind == PAIRED and k == len(other) and 0 <= slot < ring and slot not in held, (dirs, d, j, plan[i - 1])
                other.append(slot)
                held.add(slot)
            else:
                assert kind == PLAIN and slot == -1 and k == -1, (dirs, d, j, plan[i - 1], spec, ring)
    return counts


def test_plan_matches_the_brute_force_enumeration():
    paired = replays = 0
    for n in range(1, 8):
        for dirs in itertools.product((1, -1), repeat=n):
            for spec in range(0, 8):
                for ring in (1, 3, 8, 64):
                    for max_depth in (4, 10):
                        nd = min(n, max_depth)
                        c = _check(list(dirs), nd, spec, max_depth, ring)
                        paired += c[PAIRED]
                        replays += c[REPLAY]
    assert paired > 0 and replays > 0


def test_known_directions_are_all_the_plan_relies_on():
    """More directions known than doublings run (a tree that stops early): the launches that were planned are those of the longer
    tree's first doublings, and whatever was evaluated ahead for a doubling that never came is simply left over."""
    dirs = [1, -1, 1, 1, -1, 1, -1]
    full = _plan(dirs, 7, 6, 10, 64)
    short = _plan(dirs, 4, 6, 10, 64)
    assert np.array_equal(full[: len(short)], short)
    _check(dirs, 4, 6, 10, 64)


def test_no_look_ahead_no_pairing():
    for dirs in itertools.product((1, -1), repeat=6):
        plan = _plan(list(dirs), 6, 0, 10, 64)
        assert np.all(plan[:, 2] == PLAIN)


def test_a_worked_example():
    """right, left, left, right under full look-ahead: leaf (0,0) takes the left end's first leapfrog with it, which doubling 1
    replays; the five streamed leaves of doublings 1 and 2 evaluate the first five of the right end's next doubling (eight leaves);
    doubling 3 replays them and streams its last three leaves alone (nothing further is known)."""
    plan = _plan([1, -1, -1, 1], 4, 3, 10, 64)
    kinds = plan[:, 2].tolist()
    assert kinds == [PAIRED] + [REPLAY] + [PAIRED] * 5 + [REPLAY] * 5 + [PLAIN] * 3, kinds
