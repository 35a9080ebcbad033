"""The minimiser's candidate stream and session, restated in Python from the
header comment of wtf_amd/csrc/engine_minimize.h and from the rounds, skips
and selection that wtf_amd/host/minimize.cc documents; not from their code.

A base has U units: a byte buffer's bytes, a feed's packets. Levels run
k = floor(log2 U) down to 0; level k has chunks of C = 2^k units and
ceil(U / C) candidates, candidate j covering units [j * C, min(U, (j + 1) * C)).
Indices run through the levels from the largest chunk to the smallest,
ascending j within a level. REMOVE drops the range, ZERO (bytes only) clears it.
"""
from __future__ import annotations

from tests import packet_mutate_model as PM

REMOVE, ZERO = 0, 1


def levels(U):
    """[(k, n_k)] from the largest chunk to the smallest; none for U = 0."""
    if U == 0:
        return []
    top = U.bit_length() - 1
    return [(k, -(-U // (1 << k))) for k in range(top, -1, -1)]


def total(U):
    return sum(n for _, n in levels(U))


def locate(U, index):
    """(k, j, lo, hi): the level, the candidate of it, the units it covers."""
    assert 0 <= index < total(U)
    for k, n in levels(U):
        if index < n:
            lo = index << k
            return k, index, lo, min(U, lo + (1 << k))
        index -= n
    raise AssertionError


def candidate(base: bytes, op, index) -> bytes:
    _, _, lo, hi = locate(len(base), index)
    if op == REMOVE:
        return base[:lo] + base[hi:]
    assert op == ZERO
    return base[:lo] + bytes(hi - lo) + base[hi:]


def chunks_of(feed: bytes):
    """The feed's chunks, each whole (u32 Size and the Size bytes after it)."""
    out, at = [], 0
    while at < len(feed):
        size = int.from_bytes(feed[at:at + 4], "little")
        assert size >= 8 and at + 4 + size <= len(feed)
        out.append(feed[at:at + 4 + size])
        at += 4 + size
    return out


def candidate_feed(feed: bytes, index) -> bytes:
    ch = chunks_of(feed)
    _, _, lo, hi = locate(len(ch), index)
    return b"".join(ch[:lo] + ch[hi:])


# ---- the session

class ByteStream:
    """A target with a declared insert: the testcase is the base; a candidate
    the module's InsertTestcase would reject (shorter than the 4-byte head,
    longer than head + max_payload) is never ordered."""
    ops = (REMOVE, ZERO)

    def __init__(self, max_payload):
        self.max_payload = max_payload

    def units(self, base):
        return len(base)

    def make(self, base, op, index):
        return candidate(base, op, index)

    def skipped(self, base, op, index, cand):
        if op == ZERO:
            _, _, lo, hi = locate(len(base), index)
            if not any(base[lo:hi]):
                return True
        return len(cand) < 4 or (self.max_payload and len(cand) > 4 + self.max_payload)

    def testcase(self, cand):
        return cand


class FeedStream:
    """A target with a packet mutator: the base is a feed, REMOVE works over
    packets, there is no ZERO; to_testcase turns a feed into the target's file."""
    ops = (REMOVE,)

    def __init__(self, to_testcase):
        self.to_testcase = to_testcase

    def units(self, base):
        return len(chunks_of(base))

    def make(self, base, op, index):
        assert op == REMOVE
        return candidate_feed(base, index)

    def skipped(self, base, op, index, cand):
        return False

    def testcase(self, cand):
        return self.to_testcase(cand)


def minimize(base, stream, matches, max_rounds=4096):
    """The session's rounds. matches([testcase bytes]) -> [bool] runs one
    round's ordered candidates. Returns (final base, log) where log has one
    entry a round: {"op", "ordered", "skipped", "winner" (index or None),
    "base" (the round's base)}, plus counts as the session prints them."""
    log = []
    stopped = False
    for op in stream.ops:
        while True:
            if len(log) >= max_rounds:
                stopped = True
                break
            T = total(stream.units(base))
            ordered, skipped = [], 0
            for i in range(T):
                c = stream.make(base, op, i)
                if stream.skipped(base, op, i, c):
                    skipped += 1
                else:
                    ordered.append((i, c))
            got = matches([stream.testcase(c) for _, c in ordered]) if ordered else []
            assert len(got) == len(ordered)
            best = None
            for (i, c), m in zip(ordered, got):
                if not m:
                    continue
                if op == REMOVE:
                    key = len(c)
                else:
                    _, _, lo, hi = locate(len(base), i)
                    key = -sum(1 for b in base[lo:hi] if b)
                if best is None or key < best[0]:  # strict: a tie stays with the lower index
                    best = (key, i, c)
            log.append({"op": op, "ordered": len(ordered), "skipped": skipped, "base": base,
                        "winner": None if best is None else best[1]})
            if best is None:
                break
            base = best[2]
        if stopped:
            break
    counts = {"rounds": len(log), "remove_rounds": sum(r["op"] == REMOVE for r in log),
              "zero_rounds": sum(r["op"] == ZERO for r in log), "candidates": sum(r["ordered"] for r in log),
              "skipped": sum(r["skipped"] for r in log), "stopped_by_rounds": stopped}
    return base, log, counts


# ---- shared test data

def byte_base(n, salt=1):
    """n bytes with zeros among them (so that ZERO has ranges to skip)."""
    return bytes(0 if (i * 7 + salt) % 5 == 0 else (i * 31 + salt * 17 + (i >> 8)) & 0xff for i in range(n))


def feed_base(n, salt=3):
    """A feed of n packets, bodies 0..40 bytes, a body of 0 first and last."""
    lens = [0] + [((i * 13 + salt) % 41) for i in range(1, max(n - 1, 1))] + [0]
    pk = [((salt + i) % 11, i & 0xffff, lens[i] ^ (i & 3), bytes((i * 5 + j + salt) & 0xff for j in range(lens[i])))
          for i in range(n)]
    return PM.feed_of(pk)
