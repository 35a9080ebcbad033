"""The coverage-keeping rule of `minimize --keep-coverage`, restated from the
comment of wtf_amd/csrc/engine_covkeep.h (not from its code): a lane's coverage
set as an open-addressed table, the probe, missing(S, T) and what makes a
candidate keep. Also the directed tables the CPU and GPU tests share."""
from __future__ import annotations

import random

M64 = (1 << 64) - 1


def mix64(x: int) -> int:
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def cap(H: int) -> int:
    """The most values a table of H slots holds."""
    return H - H // 4


def home(v: int, H: int) -> int:
    return mix64(v) & (H - 1)


class Table:
    """A lane's set: H slots of (value, generation) and the lane's generation.
    A slot is live iff its generation is the lane's."""

    def __init__(self, H: int, g: int = 1):
        assert H & (H - 1) == 0
        self.H, self.g = H, g
        self.rip = [0] * H
        self.gen = [0] * H
        self.count = 0
        self.overflow = False

    def insert(self, v: int) -> None:
        """As the engine logs a value: the first slot that is not live from the
        value's home on, unless a live slot holding it comes first; a set of
        cap(H) values drops a value it lacks and raises the overflow flag."""
        h = home(v, self.H)
        for _ in range(self.H):
            if self.gen[h] != self.g:
                if self.count >= cap(self.H):
                    self.overflow = True
                    return
                self.rip[h], self.gen[h] = v, self.g
                self.count += 1
                return
            if self.rip[h] == v:
                return
            h = (h + 1) & (self.H - 1)

    def empty(self) -> None:
        """A restore or a collection: the generation changes, the slots stay."""
        self.g += 1
        self.count = 0
        self.overflow = False

    def has(self, v: int) -> bool:
        """The probe: a slot that is not live ends it (absent) even when it
        holds v; a live slot holding v is present; at most H slots."""
        h = home(v, self.H)
        for _ in range(self.H):
            if self.gen[h] != self.g:
                return False
            if self.rip[h] == v:
                return True
            h = (h + 1) & (self.H - 1)
        return False

    def live(self) -> list[int]:
        return sorted(self.rip[k] for k in range(self.H) if self.gen[k] == self.g)


def missing(S, T) -> int:
    """|T \\ S|"""
    S = set(S)
    return sum(1 for v in T if v not in S)


def keeps(ok: bool, error: bool, overflow: bool, miss: int) -> bool:
    return ok and not error and not overflow and miss == 0


# ---- directed tables (H = 64 in the CPU test)

def values_homed_at(H: int, slot: int, n: int, rng: random.Random, avoid=()) -> list[int]:
    """n distinct values whose home is `slot`."""
    out, avoid = [], set(avoid)
    while len(out) < n:
        v = rng.getrandbits(64)
        if home(v, H) == slot and v not in avoid and v not in out:
            out.append(v)
    return out


def tables(H: int = 64, seed: int = 0xC07EE9):
    """[(name, Table, extra target values)]: sets of 0, 1, cap - 1 and cap
    entries, one that overflowed, chains that wrap past slot H - 1, and stale
    entries of the earlier generation in the probe path. The extra values are
    ones a test should put into its targets (stale values, values in no set)."""
    rng = random.Random(seed)
    out = []
    out.append(("empty", Table(H), []))
    t = Table(H)
    t.insert(0x1400010A0)
    out.append(("one", t, []))
    for name, n in (("cap_minus_one", cap(H) - 1), ("cap", cap(H))):
        t = Table(H)
        while t.count < n:
            t.insert(0x140000000 + rng.randrange(1 << 20))
        assert not t.overflow
        out.append((name, t, []))
    t = Table(H)
    dropped = []
    while len(dropped) < 5:
        v = 0x7FF000000000 + rng.randrange(1 << 24)
        before = t.count
        t.insert(v)
        if t.count == before and not t.has(v):
            dropped.append(v)
    assert t.overflow and t.count == cap(H)
    out.append(("overflowed", t, dropped))
    # a chain of 7 values homed at H - 2: slots H - 2, H - 1, 0, 1, ...
    t = Table(H)
    wrap = values_homed_at(H, H - 2, 7, rng)
    for v in wrap:
        t.insert(v)
    assert [t.rip[k] for k in (H - 2, H - 1, 0, 1, 2, 3, 4)] == wrap
    out.append(("wrap", t, values_homed_at(H, H - 2, 3, rng, avoid=wrap)))  # walk the whole chain, then absent
    # stale entries: generation 1 puts a, v1, v2 in a chain at slot 9; the set
    # empties; generation 2 puts w (home 9) at slot 9. v1 and v2 still sit in
    # slots 10 and 11 with the old generation: the probe for v1 passes the
    # live slot 9 and ends at slot 10, absent, though the slot holds v1
    t = Table(H)
    a, v1, v2 = values_homed_at(H, 9, 3, rng)
    for v in (a, v1, v2):
        t.insert(v)
    t.empty()
    w = values_homed_at(H, 9, 1, rng, avoid=(a, v1, v2))[0]
    t.insert(w)
    assert t.rip[10] == v1 and t.gen[10] != t.g and t.rip[9] == w
    out.append(("stale_in_path", t, [a, v1, v2]))
    # the same with a wrapped chain and a stale value at its own home slot
    t = Table(H)
    old = values_homed_at(H, H - 1, 4, rng)
    for v in old:
        t.insert(v)
    t.empty()
    new = values_homed_at(H, H - 1, 2, rng, avoid=old)
    for v in new:
        t.insert(v)
    assert t.rip[1] == old[2] and t.gen[1] != t.g
    out.append(("stale_wrap", t, old))
    # a random fill over a table full of stale entries of the same values
    t = Table(H)
    pool = [0x140001000 + 3 * k for k in range(cap(H))]
    for v in pool:
        t.insert(v)
    t.empty()
    for v in rng.sample(pool, 20):
        t.insert(v)
    out.append(("stale_same_values", t, pool))
    return out


def targets(union, extras, rng: random.Random, sizes=(0, 1, 63, 64, 65, 200)):
    """One sorted unique target of each size: drawn from `union` (values some
    set holds) and `extras`, topped up with values in no set."""
    union, extras = sorted(set(union)), sorted(set(extras))
    out = []
    for n in sizes:
        take = set(rng.sample(extras, min(len(extras), n // 3)))
        take |= set(rng.sample(union, min(len(union), n - len(take))))
        while len(take) < n:
            take.add(0x6000000000000000 | rng.getrandbits(48))  # in no set
        out.append(sorted(take))
    return out
