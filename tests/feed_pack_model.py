"""The layout of a packed feed read-back (wtfgpu_read_feeds_packed), restated
from the comment at the head of wtf_amd/csrc/engine_feedpack.h, not from its
code. A feed is `bytes`; None is a listed lane without one."""
NO_FEED = 0xFFFFFFFF
STRIDE = 16384


def pad16(n):
    return 0 if n == NO_FEED else (n + 15) // 16 * 16


def offsets(lens):
    """(offs, total): the exclusive sum, in list order, of the padded lengths (Python integers: no width)."""
    offs, at = [], 0
    for n in lens:
        offs.append(at)
        at += pad16(n)
    return offs, at


def pack(feeds):
    """(lens, offs, total, bytes) of a list of feeds."""
    lens = [NO_FEED if f is None else len(f) for f in feeds]
    offs, total = offsets(lens)
    out = b"".join(b"" if f is None else f + bytes(pad16(len(f)) - len(f)) for f in feeds)
    assert len(out) == total
    return lens, offs, total, out


def chunk_len(size_word, stride=STRIDE):
    return min(size_word, stride - 4)


def whole_len(length, stride=STRIDE):
    return min(length, stride)


def padding_is_zero(lens, offs, total, buf):
    """Every byte of buf[:total] that is no lane's byte is zero, and the places tile the buffer."""
    at = 0
    for n, o in zip(lens, offs):
        if o != at:
            return False
        if n == NO_FEED:
            continue
        if any(buf[o + n:o + pad16(n)]):
            return False
        at = o + pad16(n)
    return at == total == len(buf)
