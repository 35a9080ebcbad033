"""TEST INFRASTRUCTURE ONLY: the analyzer's rule (`wtfgpu analyze`), restated
from the head comment of wtf_amd/csrc/engine_analyze.h, not from its code.

Positions: every byte of a byte buffer; every byte of a feed except the four
bytes of each chunk's u32 Size (framing). Four variants a position:
b ^ 0xFF, b ^ 0x01, b + 0x10, b - 0x10 (mod 256). index = 4 * p + v; the
candidate is the base with byte p replaced, the same size.

sig(S) = (sum of mix64(v) over S mod 2^64, |S|). An outcome is (kind, crash
name, sig, size, overflow); two are the same iff neither overflowed and the
other parts are equal. A position's class comes from how many of its four
variants' outcomes differ from the base's, and whether the four are the same
as each other."""
import struct

from tests.covkeep_model import M64, mix64

VARIANTS = 4
NONE, MINOR, FIXED, VARIABLE, FRAMING = ".", "m", "F", "V", "#"


def variant(b: int, v: int) -> int:
    return [b ^ 0xFF, b ^ 0x01, (b + 0x10) & 0xFF, (b - 0x10) & 0xFF][v]


def total(U: int) -> int:
    return VARIANTS * U


def candidate(base: bytes, index: int) -> bytes:
    """Candidate `index` of a base (a byte buffer, or a feed's chunk bytes)."""
    p, v = divmod(index, VARIANTS)
    assert p < len(base)
    return base[:p] + bytes([variant(base[p], v)]) + base[p + 1:]


# ---- feeds

def make_feed(packets) -> bytes:
    """Chunks of (command, id, bodysize, body): u32 Size, u32 Command, u16 Id,
    u16 BodySize, Body; Size counts what follows it."""
    out = b""
    for cmd, pid, bodysize, body in packets:
        out += struct.pack("<IIHH", 8 + len(body), cmd, pid, bodysize) + body
    return out


def chunk_offsets(feed: bytes) -> list[int]:
    """coff[0 .. P]: each chunk's first byte, then the feed's length."""
    at, off = 0, []
    while at < len(feed):
        off.append(at)
        at += 4 + struct.unpack_from("<I", feed, at)[0]
    assert at == len(feed)
    return off + [len(feed)]


def framing(feed: bytes) -> list[bool]:
    """Per position: is it one of a chunk's four Size bytes?"""
    out = [False] * len(feed)
    for at in chunk_offsets(feed)[:-1]:
        for k in range(4):
            out[at + k] = True
    return out


def fields(feed: bytes) -> list[tuple[int, str]]:
    """Per position: (packet, field)."""
    off = chunk_offsets(feed)
    out = []
    for k in range(len(off) - 1):
        for p in range(off[k], off[k + 1]):
            d = p - off[k]
            out.append((k, "size" if d < 4 else "command" if d < 8 else "id" if d < 10 else "bodysize" if d < 12
                        else "body"))
    return out


def indices(base: bytes, feed: bool = False) -> list[int]:
    """Every candidate index of a base, ascending."""
    fr = framing(base) if feed else [False] * len(base)
    return [VARIANTS * p + v for p in range(len(base)) if not fr[p] for v in range(VARIANTS)]


# ---- signatures, outcomes, classes

def sig(values) -> tuple[int, int]:
    """(sum, size) of a collection of distinct values."""
    values = list(values)
    assert len(set(values)) == len(values)
    return sum(mix64(v) for v in values) & M64, len(values)


def outcome(kind: str, name: str = "", values=(), overflow: bool = False):
    """kind: ok, crash, timedout, cr3, error."""
    s, n = sig(values)
    return (kind, name if kind == "crash" else "", s, n, overflow)


def same(a, b) -> bool:
    return not a[4] and not b[4] and a[:4] == b[:4]


def classify(base, variants) -> str:
    assert len(variants) == VARIANTS
    d = sum(not same(base, v) for v in variants)
    if d == 0:
        return NONE
    if d < VARIANTS:
        return MINOR
    if all(same(variants[a], variants[b]) for a in range(VARIANTS) for b in range(a + 1, VARIANTS)):
        return FIXED
    return VARIABLE


def ranges(classes: str, feed: bytes | None = None) -> list[dict]:
    """The maximal runs of a class string; for a feed a run also stays within
    one packet's field."""
    f = fields(feed) if feed is not None else None
    out, lo = [], 0
    while lo < len(classes):
        hi = lo + 1
        while hi < len(classes) and classes[hi] == classes[lo] and (f is None or f[hi] == f[lo]):
            hi += 1
        r = {"lo": lo, "hi": hi, "class": classes[lo]}
        if f is not None:
            r["packet"], r["field"] = f[lo]
        out.append(r)
        lo = hi
    return out
