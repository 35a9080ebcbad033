"""The device mutator's stream in plain Python, written from the definition in
the comment at the top of wtf_amd/csrc/engine_mutate.h (not from its code):
(seed, index, corpus, ncorpus, max_len) -> bytes.

mutate() also reports which operator succeeded and which failed on the way,
which tests/test_device_mutate.py uses to assert its own reach."""
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
OPS = ["EraseBytes", "InsertByte", "InsertRepeatedBytes", "ChangeByte", "ChangeBit", "ShuffleBytes",
       "ChangeASCIIInteger", "ChangeBinaryInteger", "CopyPart", "CrossOver"]
SPECIAL = b"!*'();:@&=+$,/?%#[]012Az-`~.\xff\x00"
assert len(SPECIAL) == 30
DIGITS = frozenset(b"0123456789")


def mix(z):
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


class Rng:
    def __init__(self, seed, index):
        self.s = mix((mix((seed + G) & M64) + index) & M64)

    def next(self):
        self.s = (self.s + G) & M64
        return mix(self.s)

    def R(self, n):
        if n == 0:
            return 0
        if n <= 1 << 32:
            return ((self.next() >> 32) * n) >> 32
        return self.next() % n

    def ch(self):
        return self.R(256) if self.R(2) else SPECIAL[self.R(30)]


def _copy_part_of(g, b, frm):
    S, FS = len(b), len(frm)
    to = g.R(S)
    n = min(g.R(S - to) + 1, FS)
    fb = g.R(FS - n + 1)
    return b[:to] + frm[fb:fb + n] + b[to + n:]


def _insert_part_of(g, b, frm, Max):
    S, FS = len(b), len(frm)
    if S >= Max:
        return None
    n = g.R(min(Max - S, FS)) + 1
    fb = g.R(FS - n + 1)
    at = g.R(S + 1)
    return b[:at] + frm[fb:fb + n] + b[at:]


def _apply(g, op, b, p, Max):
    """The result, or None when the operator does not apply."""
    S = len(b)
    if op == 0:
        if S <= 1:
            return None
        n = g.R(S // 2) + 1
        at = g.R(S - n + 1)
        return b[:at] + b[at + n:]
    if op == 1:
        if S >= Max:
            return None
        at = g.R(S + 1)
        return b[:at] + bytes([g.ch()]) + b[at:]
    if op == 2:
        if S + 3 >= Max:
            return None
        n = g.R(min(Max - S, 128) - 2) + 3
        at = g.R(S + 1)
        c = g.R(256) if g.R(2) else (0 if g.R(2) else 255)
        return b[:at] + bytes([c]) * n + b[at:]
    if op == 3:
        if S == 0:
            return None
        at = g.R(S)
        return b[:at] + bytes([g.ch()]) + b[at + 1:]
    if op == 4:
        if S == 0:
            return None
        at = g.R(S)
        return b[:at] + bytes([b[at] ^ (1 << g.R(8))]) + b[at + 1:]
    if op == 5:
        if S == 0:
            return None
        n = g.R(min(S, 8)) + 1
        at = g.R(S - n)
        w = bytearray(b[at:at + n])
        for i in range(n - 1, 0, -1):
            j = g.R(i + 1)
            w[i], w[j] = w[j], w[i]
        return b[:at] + bytes(w) + b[at + n:]
    if op == 6:
        if S == 0:
            return None
        B = g.R(S)
        while B < S and b[B] not in DIGITS:
            B += 1
        if B == S:
            return None
        E = B
        while E < S and b[E] in DIGITS:
            E += 1
        v = int(b[max(B, E - 70):E]) & M64  # 2^64 divides 10^64: older digits add nothing
        c = g.R(5)
        if c == 0:
            v = (v + 1) & M64
        elif c == 1:
            v = (v - 1) & M64
        elif c == 2:
            v //= 2
        elif c == 3:
            v = (v * 2) & M64
        else:
            v = g.R((v * v) & M64)
        width = E - B
        text = b"%0*d" % (width, v)
        return b[:B] + text[len(text) - width:] + b[E:]
    if op == 7:
        W = 1 << g.R(4)
        if S < W:
            return None
        off = g.R(S - W + 1)
        mask = (1 << (8 * W)) - 1
        if off < 64 and g.R(4) == 0:
            v = S & mask
            if g.R(2):
                v = int.from_bytes(v.to_bytes(W, "little"), "big")
        else:
            v = int.from_bytes(b[off:off + W], "little")
            a = g.R(21) - 10
            if g.R(2):
                v = int.from_bytes(b[off:off + W], "big")
                v = (v + a) & mask
                v = int.from_bytes(v.to_bytes(W, "big"), "little")
            else:
                v = (v + a) & mask
            if a == 0 or g.R(2):
                v = ~v & mask
        return b[:off] + v.to_bytes(W, "little") + b[off + W:]
    if op == 8:
        if S == 0:
            return None
        if S == Max or g.R(2):
            return _copy_part_of(g, b, b)
        return _insert_part_of(g, b, b, Max)
    if S == 0 or len(p) == 0:
        return None
    if g.R(2) == 0:
        return _copy_part_of(g, b, p)
    return _insert_part_of(g, b, p, Max)


def mutate(seed, index, corpus, ncorpus, max_len):
    """(bytes, op that succeeded or None, [ops that failed before it])."""
    g = Rng(seed, index)
    b = corpus[g.R(ncorpus)][:max_len]
    p = corpus[g.R(ncorpus)]
    failed = []
    for _ in range(100):
        op = g.R(10)
        out = _apply(g, op, b, p, max_len)
        if out is not None:
            assert 0 < len(out) <= max_len
            return out, op, failed
        failed.append(op)
    return b, None, failed


def testcase(seed, index, corpus, ncorpus, max_len) -> bytes:
    return mutate(seed, index, corpus, ncorpus, max_len)[0]


# ---- the corpora the CPU and the GPU tests share
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 1028, 16380]
KINDS = ["zero", "ff", "digits", "random"]
MAX_LENS = [4, 5, 64, 1028, 16380]
NCORPUS = [1, 2, 10]


def _content(kind, n, salt):
    if kind == "zero":
        return bytes(n)
    if kind == "ff":
        return b"\xff" * n
    g = Rng(0xC0, salt)
    if kind == "digits":  # a leading '-', then decimal digits
        return (b"-" + bytes(0x30 + g.R(10) for _ in range(n)))[:n]
    return bytes(g.R(256) for _ in range(n))


def corpora():
    """{name: 10 entries}: one corpus per kind of content, the lengths rotated
    so that the one- and two-entry prefixes differ between them, and one that
    mixes the kinds."""
    out = {}
    for k, kind in enumerate(KINDS):
        rot = LENGTHS[2 * k:] + LENGTHS[:2 * k]
        out[kind] = [_content(kind, n, 16 * k + i) for i, n in enumerate(rot)]
    rot = LENGTHS[7:] + LENGTHS[:7]
    out["mixed"] = [_content(KINDS[(i + 2) % 4], n, 64 + i) for i, n in enumerate(rot)]
    return out


def pack(entries):
    """(arena bytes, offsets) as wtfmut::Corpus and the device arena hold them."""
    off = [0]
    for e in entries:
        off.append(off[-1] + len(e))
    return b"".join(entries), off
