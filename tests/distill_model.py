"""The corpus distiller's rule, restated from the comment at the top of
wtf_amd/csrc/engine_distill.h (not from its code), and the set builders the
distill tests share.

There are n sets in rank order, each a strictly ascending list of 64-bit
values, each with an `eligible` flag.

    covered = {}
    loop:
      g_i = |S_i \\ covered| for every eligible i not yet taken
      if max g_i == 0: stop
      take the lowest i whose g_i is the maximum; record (i, g_i); covered |= S_i

The output is the taken indices in the order taken, their gains, and
`universe`: the number of distinct values over the eligible sets."""
from __future__ import annotations

import random

import numpy as np

SIZES = [0, 1, 63, 64, 65, 300, 8192]  # set sizes mixed inside one call
COUNTS = [1, 63, 64, 65, 257]          # sets a call
UNIVERSES = [1, 31, 32, 33, 64, 65, 4097]  # bitmap word and dword edges


def distill(sets, eligible=None):
    """(index, gain, universe) of the rule, every gain counted in every round."""
    n = len(sets)
    elig = [True] * n if eligible is None else [bool(e) for e in eligible]
    live = [i for i in range(n) if elig[i]]
    allv = sorted({int(v) for i in live for v in sets[i]})
    ident = {v: k for k, v in enumerate(allv)}
    ids = {i: np.array([ident[int(v)] for v in sets[i]], dtype=np.int64) for i in live}
    covered = np.zeros(len(allv) + 1, dtype=bool)
    index, gain = [], []
    while True:
        best, best_i = 0, None
        for i in live:
            g = int(np.count_nonzero(~covered[ids[i]]))
            if g > best:  # strictly: the lowest index among equals stays
                best, best_i = g, i
        if best == 0:
            break
        index.append(best_i)
        gain.append(best)
        covered[ids[best_i]] = True
        live.remove(best_i)
    return index, gain, len(allv)


def check_properties(sets, eligible, index, gain, universe):
    """What the header promises of any output of the rule."""
    n = len(sets)
    elig = [True] * n if eligible is None else [bool(e) for e in eligible]
    assert len(index) == len(gain) == len(set(index)) and all(elig[i] for i in index)
    assert all(g >= 1 for g in gain) and all(a >= b for a, b in zip(gain, gain[1:]))
    union = set().union(*[set(map(int, sets[i])) for i in range(n) if elig[i]]) if any(elig) else set()
    taken = set().union(*[set(map(int, sets[i])) for i in index]) if index else set()
    assert taken == union and universe == len(union) == sum(gain)
    # idempotence: the taken sets alone, in the same relative order, are all taken, in the same order
    order = sorted(index)
    again, again_gain, _ = distill([sets[i] for i in order])
    assert [order[k] for k in again] == index and again_gain == gain


# ---- values

def pool(count: int, salt: int = 0) -> list[int]:
    """`count` distinct 64-bit values, ascending: small dense runs (neighbouring
    ids share a bitmap word), values at and above 2^63 (a signed sort or
    compare misplaces them), and pairs that differ only above bit 32 (a
    truncated compare merges them)."""
    out = set()
    k = 0
    while len(out) < count:
        kind = k % 4
        if kind == 0:
            out.add(0x1000 + salt + k)
        elif kind == 1:
            out.add((1 << 63) + salt + k)
        elif kind == 2:
            out.add(((k + 1) << 32) | 7)
        else:
            out.add(0xFFFFFFFF00000000 + salt + k)
        k += 1
    return sorted(out)


def subset(rng: random.Random, values: list[int], size: int) -> list[int]:
    return sorted(rng.sample(values, size))


def mixed(n: int, seed: int) -> list[list[int]]:
    """n sets whose sizes cycle through SIZES (from a rotating start, so every
    n sees every size it can), drawn from a pool of 12,000 values."""
    rng = random.Random(seed)
    values = pool(12000, seed)
    return [subset(rng, values, SIZES[(i + seed) % len(SIZES)]) for i in range(n)]


def over_universe(U: int, seed: int, n: int = 40) -> list[list[int]]:
    """n sets over exactly U values: random subsets, one dense run of up to 32
    neighbouring values, and singletons of the first and the last value."""
    rng = random.Random(seed * 7919 + U)
    values = pool(U, seed)
    sets = [set(subset(rng, values, rng.randint(0, min(U, 48)))) for _ in range(n - 3)]
    for v in set(values).difference(*sets):  # every value is in some set: the universe is U
        rng.choice(sets).add(v)
    sets = [sorted(s) for s in sets]
    at = rng.randrange(max(U - 32, 0) + 1)
    sets.insert(n // 2, values[at:at + 32])
    sets += [[values[0]], [values[-1]]]
    return sets


def identical(copies: int = 5) -> list[list[int]]:
    """The same set `copies` times after a smaller one: index 1 wins, alone."""
    values = pool(70)
    return [values[:9]] + [values[:]] * copies


def far_tie() -> list[list[int]]:
    """100 sets; 5 and 70 (another wave and another block of the gain kernel)
    are disjoint and the largest, of equal size: 5 is taken, then 70."""
    rng = random.Random(570)
    values = pool(400)
    sets = [subset(rng, values[:200], rng.randint(0, 20)) for _ in range(100)]
    sets[5], sets[70] = values[200:230], values[300:330]
    return sets


def chain(n: int = 65) -> list[list[int]]:
    """S_i is a proper subset of S_{i+1}: only the last is taken."""
    values = pool(n)
    return [values[:i + 1] for i in range(n)]


def order_dependent() -> list[list[int]]:
    """The classic instance: Y is larger than Z, but once X is taken Y adds 3
    and Z adds 4, so the picks are X, Z, Y."""
    v = pool(30)
    return [v[4:11], v[20:24], v[0:8]]  # Y, Z, X in rank order


def singletons(n: int = 300) -> list[list[int]]:
    """n disjoint sets of one value: n rounds of gain 1, in index order."""
    return [[v] for v in pool(n)]


def random_instance(rng: random.Random):
    """A small instance with many ties: (sets, eligible or None)."""
    n = rng.randint(0, 20)
    values = pool(rng.randint(1, 40), rng.randrange(1000))
    sets = [subset(rng, values, rng.randint(0, min(len(values), 12))) for _ in range(n)]
    eligible = None if rng.random() < 0.3 else [rng.random() < 0.8 for _ in range(n)]
    return sets, eligible


def shapes():
    """(name, sets, eligible) of every directed shape."""
    for n in COUNTS:
        yield f"mixed{n}", mixed(n, n), None
    for U in UNIVERSES:
        yield f"universe{U}", over_universe(U, 3), None
    yield "identical", identical(), None
    yield "far_tie", far_tie(), None
    yield "chain", chain(), None
    yield "order_dependent", order_dependent(), None
    yield "singletons", singletons(), None
    yield "all_ineligible", over_universe(65, 5), [False] * 40
    yield "eligible_mixed", mixed(65, 9), [i % 3 != 1 for i in range(65)]
    yield "empty_sets", [[], [], []], None
    yield "none", [], None


def synthetic(n: int, mean: int, universe: int, seed: int):
    """A large instance for measurements, as (offsets, values): n sets of about
    `mean` values each (sizes uniform in [mean / 2, 3 mean / 2], duplicates of
    a draw dropped), drawn from `universe` values spread over 64 bits."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(mean // 2, mean + mean // 2 + 1, size=n)
    sets = []
    for s in sizes:
        ids = np.unique(rng.integers(0, universe, size=int(s), dtype=np.uint64))
        sets.append(ids * np.uint64(0x9E3779B97F4A7C15 // universe | 1))  # ascending still: no wrap below 2^64
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in sets], dtype=np.uint64)
    return off, np.concatenate(sets)


def flatten(sets):
    """(offsets, values) as numpy arrays, the layout of wtfgpu_distill."""
    off = np.zeros(len(sets) + 1, dtype=np.uint64)
    if sets:
        off[1:] = np.cumsum([len(s) for s in sets], dtype=np.uint64)
    flat = [v for s in sets for v in s]
    return off, np.array(flat if flat else [0], dtype=np.uint64)
