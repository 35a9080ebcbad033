"""The device packet mutator's stream in plain Python, written from the
definition in the comment at the top of wtf_amd/csrc/engine_mutate_packets.h
(not from its code): (seed, index, corpus of feeds, ncorpus, params) -> feed.

A feed is handled as a list of packets (command, id, body_size, body) and
written back as chunks; mutate() also reports what the testcase was, which
tests/test_device_packets.py uses to assert its own reach. The generator (mix,
s0, next, R) is tests/mutate_model.py's, as the header reuses engine_mutate.h's."""
import struct

from tests.mutate_model import G, M64, Rng, mix  # noqa: F401

WHAT = ["Generate", "Insert", "InsertEmpty", "InsertTooMany", "InsertTooLong", "CopyId", "CopyCommand",
        "CopyBodySize", "CopyBody", "CopyEmpty", "CopyBodyTooLong", "Erase", "EraseEmpty"]
(GENERATE, INSERT, INSERT_EMPTY, INSERT_TOO_MANY, INSERT_TOO_LONG, COPY_ID, COPY_COMMAND, COPY_BODY_SIZE, COPY_BODY,
 COPY_EMPTY, COPY_BODY_TOO_LONG, ERASE, ERASE_EMPTY) = range(13)

MAX_FEED = 16384
# GenMaxPackets, GenCommands, GenMaxBody, FlipOneIn, InsertMaxPackets (tlv's), then MaxFeed
TLV = (10, 11, 100, 3, 10)


def chunk(command, id_, body_size, body):
    return struct.pack("<IIHH", 8 + len(body), command & 0xffffffff, id_ & 0xffff, body_size & 0xffff) + bytes(body)


def feed_of(packets):
    return b"".join(chunk(*p) for p in packets)


def packets_of(feed):
    """The packets of a valid feed; None when the chunks do not tile it, a Size
    is below 8, or it is longer than MAX_FEED."""
    if len(feed) > MAX_FEED:
        return None
    out, at = [], 0
    while at < len(feed):
        if len(feed) - at < 4:
            return None
        size, = struct.unpack_from("<I", feed, at)
        if size < 8 or size > len(feed) - at - 4:
            return None
        command, id_, body_size = struct.unpack_from("<IHH", feed, at + 4)
        out.append((command, id_, body_size, feed[at + 12:at + 4 + size]))
        at += 4 + size
    return out


def draw(s0, k, n):
    """The k-th draw, mapped as R(n) maps it."""
    return ((mix((s0 + k * G) & M64) >> 32) * n) >> 32


def mutate(seed, index, corpus, ncorpus, params=TLV, max_feed=MAX_FEED):
    """(feed bytes, what) of testcase `index` over corpus[:ncorpus] (a list of feeds)."""
    gen_max_packets, gen_commands, gen_max_body, flip_one_in, insert_max_packets = params
    g = Rng(seed, index)
    s0 = g.s
    if g.R(5) == 4:
        n = g.R(gen_max_packets) + 1
        packets = []
        for p in range(n):
            k = 3 + 4 * p
            command, length = draw(s0, k, gen_commands), draw(s0, k + 1, gen_max_body + 1)
            f, b = draw(s0, k + 2, flip_one_in), draw(s0, k + 3, 16)
            body_size = (length & 0xffff) ^ ((1 << b) if f == 0 else 0)
            packets.append((command, p, body_size, bytes(length)))
        return feed_of(packets), GENERATE
    base = corpus[g.R(ncorpus)]
    op = g.R(3)
    pk = packets_of(base)
    P = len(pk)
    if P == 0:
        return base, (INSERT_EMPTY, COPY_EMPTY, ERASE_EMPTY)[op]
    if op == 0:
        if P > insert_max_packets:
            return base, INSERT_TOO_MANY
        frm, to = g.R(P), g.R(P + 1)
        out = feed_of(pk[:to] + [pk[frm]] + pk[to:])
        return (out, INSERT) if len(out) <= max_feed else (base, INSERT_TOO_LONG)
    if op == 1:
        src, dst, f = g.R(P), g.R(P), g.R(4)
        command, id_, body_size, body = pk[dst]
        if f == 0:
            id_ = pk[src][1]
        elif f == 1:
            command = pk[src][0]
        elif f == 2:
            body_size = pk[src][2]
        else:
            body = pk[src][3]
        out = feed_of(pk[:dst] + [(command, id_, body_size, body)] + pk[dst + 1:])
        if len(out) > max_feed:
            return base, COPY_BODY_TOO_LONG
        return out, COPY_ID + f
    k = g.R(P)
    return feed_of(pk[:k] + pk[k + 1:]), ERASE


def testcase(seed, index, corpus, ncorpus, params=TLV):
    return mutate(seed, index, corpus, ncorpus, params)[0]


def pack(corpus):
    """The corpus as wtfgpu_corpus_add_feed lays it out: (arena bytes, entry
    offsets). Entry: u32 P, u32 coff[P + 1], the chunks, zeros to a multiple of 4."""
    arena, off = b"", [0]
    for feed in corpus:
        pk = packets_of(feed)
        assert pk is not None
        coff, at = [], 0
        for p in pk:
            coff.append(at)
            at += 12 + len(p[3])
        coff.append(at)
        assert at == len(feed)
        e = struct.pack(f"<I{len(coff)}I", len(pk), *coff) + feed
        arena += e + bytes(-len(e) % 4)
        off.append(len(arena))
    return arena, off


def _body(n, salt):
    return bytes((salt * 37 + i * 11 + (i >> 8)) & 0xff for i in range(n))


def corpus():
    """The test corpus. Packet counts 0, 1, 2, 10, 11, 12 and 64; body lengths
    0, 1, 2, 3, 5, 100, 4083 and 4084 (a chunk of exactly 0x1000 bytes); an
    entry whose insert-copy can give exactly 16384 bytes (chunks of 5460 and
    5464 bytes, the first copied) and one whose insert-copy gives 16385 (5461
    and 5463: copying either does); an entry of two 8192-byte chunks, which no
    insert-copy fits; one whose copy-body can pass 16384."""
    def pkts(n, lens, salt):
        return [((salt + i) % 13, (salt * 7 + i) & 0xffff, (lens[i % len(lens)] ^ (i << 3)) & 0xffff,
                 _body(lens[i % len(lens)], salt + i)) for i in range(n)]
    c = [
        feed_of([]),                                     # P = 0
        feed_of(pkts(1, [5], 1)),
        feed_of(pkts(2, [0, 1], 2)),
        feed_of(pkts(10, [2, 3, 100], 3)),
        feed_of(pkts(11, [3, 0, 5], 4)),
        feed_of(pkts(12, [1, 2], 5)),
        feed_of(pkts(64, [0, 1, 2, 3, 5], 6)),
        feed_of(pkts(3, [4083, 4084, 100], 7)),          # chunks of 0xfff and 0x1000 bytes
        feed_of(pkts(2, [5460 - 12, 5464 - 12], 8)),     # 10924 bytes: + 5460 = 16384, + 5464 = 16388
        feed_of(pkts(2, [5461 - 12, 5463 - 12], 9)),     # 10924 bytes: + 5461 = 16385
        feed_of(pkts(2, [8192 - 12, 8192 - 12], 10)),    # 16384 bytes: a base that fills the region
        feed_of(pkts(3, [10000, 3000, 0], 11)),          # copy-body of the first over the second: 20036
    ]
    assert [len(packets_of(f)) for f in c] == [0, 1, 2, 10, 11, 12, 64, 3, 2, 2, 2, 3]
    assert len(c[8]) == 10924 and len(c[10]) == 16384
    return c


# ncorpus: 1 (the empty feed alone), then growing to the full corpus
NCORPUS = [1, 2, 3, 5, 7, 8, 9, 10, 11, 12]
