"""Aeron term-buffer framing, the publish side, for the tests of sbe_term_append: the offer loop
restated in Python (append), hand-written cases with the expected bytes spelled out, the cases the
GPU and host tests share, and the case file the C++ programs of tests/termappend read.

The frame layer is third-party Aeron (absent from the reference tree), so the loop is restated from
ExclusivePublication::offer -> ExclusiveTermAppender::appendUnfragmentedMessage /
appendFragmentedMessage / handleEndOfLogCondition and the data-frame layout (termscan_lib), not
compiled.  termscan_lib.framed_records is the independent builder it is held to."""
import os
import struct

import numpy as np

import sbe_testlib as T

DIR = os.path.join(T.ROOT, "tests", "termappend")
END, LIMIT, TRIPPED, TOO_LONG, BAD_RECORD = range(5)
HDR = 32
BEGIN, ENDF = 0x80, 0x40
SENTINEL = 0xA5
HEADER = (1, 7, 1001, 3, 0)          # version, session, stream, term, term_offset_base: termscan_lib.header's
NO_LIMIT = (1 << 64) - 1
MAX_LEN = 1 << 30


def align(n):
    return (n + 31) & ~31


def required(length, mtu):
    maxp = mtu - HDR
    if length <= maxp:
        return align(HDR + length)
    rem = length % maxp
    return (length // maxp) * mtu + (align(HDR + rem) if rem else 0)


def frame_header(length, flags, ftype, term_offset, header):
    version, session, stream, term, _ = header
    return struct.pack("<iBBHiiiiq", length, version, flags, ftype, term_offset, session, stream, term, 0)


def append_offsets(block, start, data, rec_off, mtu=1408, header=HEADER, limit=None, max_message_length=None):
    """The offer loop over records data[rec_off[i]:rec_off[i+1]] into `block` (bytes) from `start`.
    Returns dict(block, appended, next, payload, stop, rec_tail)."""
    out = bytearray(block)
    nb = len(out)
    limit = NO_LIMIT if limit is None else limit
    max_len = MAX_LEN if max_message_length is None else max_message_length
    maxp = mtu - HDR
    base = header[4]
    tail, tails, stop = start, [], END
    n = len(rec_off) - 1
    for i in range(n):
        lo, hi = int(rec_off[i]), int(rec_off[i + 1])
        if hi < lo or hi > len(data):
            stop = BAD_RECORD
            break
        if tail >= limit:
            stop = LIMIT
            break
        if hi - lo > max_len:
            stop = TOO_LONG
            break
        rec = bytes(data[lo:hi])
        if tail + required(len(rec), mtu) > nb:
            if tail < nb:
                out[tail: tail + HDR] = frame_header(nb - tail, BEGIN | ENDF, 0, base + tail, header)
            tail = nb
            stop = TRIPPED
            break
        parts = [rec[k: k + maxp] for k in range(0, len(rec), maxp)] or [b""]
        for t, p in enumerate(parts):
            fl = (BEGIN if t == 0 else 0) | (ENDF if t == len(parts) - 1 else 0)
            size = align(HDR + len(p))
            out[tail: tail + size] = frame_header(HDR + len(p), fl, 1, base + tail, header) + p + bytes(size - HDR - len(p))
            tail += size
        tails.append(tail)
    k = len(tails)
    return dict(block=bytes(out), appended=k, next=tail, payload=int(rec_off[k]) - int(rec_off[0]) if n >= 0 else 0,
                stop=stop, rec_tail=tails)


def pack(records, lead=0):
    """(data, rec_off) of records laid back to back behind `lead` filler bytes."""
    off = [lead]
    for r in records:
        off.append(off[-1] + len(r))
    return bytes([0xEE]) * lead + b"".join(records), off


def append(block, start, records, mtu=1408, header=HEADER, limit=None, max_message_length=None):
    data, off = pack(records)
    return append_offsets(block, start, data, off, mtu, header, limit, max_message_length)


def rec(n, seed=0):
    """n payload bytes, none of them zero or the sentinel (so a missing or a stray byte shows)."""
    return bytes(1 + (seed * 17 + 7 * j) % 0xA0 for j in range(n))


def sentinel(n):
    return bytes([SENTINEL]) * n


class Case:
    """One call: a sentinel-filled block of block_bytes, records as (data, rec_off)."""

    def __init__(self, name, block_bytes, start, data, rec_off, mtu=1408, header=HEADER, limit=None,
                 max_message_length=None):
        self.name, self.block_bytes, self.start, self.data, self.rec_off = name, block_bytes, start, data, list(rec_off)
        self.mtu, self.header, self.limit, self.max_message_length = mtu, header, limit, max_message_length

    @classmethod
    def of(cls, name, block_bytes, start, records, lead=0, **kw):
        data, off = pack(records, lead)
        return cls(name, block_bytes, start, data, off, **kw)

    def expect(self):
        return append_offsets(sentinel(self.block_bytes), self.start, self.data, self.rec_off, self.mtu, self.header,
                              self.limit, self.max_message_length)


# ---- hand cases: (Case, expected block bytes, appended, next, payload, stop, rec_tail), all written out ----
def _hand_cases():
    S = sentinel
    H = lambda length, flags, ftype, off: struct.pack("<iBBHiiiiq", length, 1, flags, ftype, off, 7, 1001, 3, 0)
    out = []

    def add(case, block, appended, nxt, payload, stop, tails):
        out.append((case, block, appended, nxt, payload, stop, tails))

    add(Case.of("one 3-byte record", 128, 0, [b"abc"]),
        H(35, 0xC0, 1, 0) + b"abc" + bytes(29) + S(64), 1, 64, 3, END, [64])
    add(Case.of("a 0-byte record", 64, 32, [b""]),
        S(32) + H(32, 0xC0, 1, 32), 1, 64, 0, END, [64])
    a, b, c = rec(32, 1), rec(33, 2), rec(64, 3)
    add(Case.of("maxp, maxp + 1 and 2 maxp at mtu 64", 64 + 128 + 128 + 32, 0, [a, b, c], mtu=64),
        H(64, 0xC0, 1, 0) + a
        + H(64, 0x80, 1, 64) + b[:32] + H(33, 0x40, 1, 128) + b[32:] + bytes(31)
        + H(64, 0x80, 1, 192) + c[:32] + H(64, 0x40, 1, 256) + c[32:] + S(32),
        3, 320, 129, END, [64, 192, 320])
    add(Case.of("a trip with a padding header", 128, 0, [b"abc", rec(40)]),
        H(35, 0xC0, 1, 0) + b"abc" + bytes(29) + H(64, 0xC0, 0, 64) + S(32), 1, 128, 3, TRIPPED, [64])
    add(Case.of("a trip at the end of the block: nothing written", 64, 0, [b"abc", b"d"]),
        H(35, 0xC0, 1, 0) + b"abc" + bytes(29), 1, 64, 3, TRIPPED, [64])
    add(Case.of("an exact fit is not a trip", 64, 0, [b"abc"]),
        H(35, 0xC0, 1, 0) + b"abc" + bytes(29), 1, 64, 3, END, [64])
    add(Case.of("limit", 256, 0, [b"abc", b"d", b"e"], limit=64),
        H(35, 0xC0, 1, 0) + b"abc" + bytes(29) + S(192), 1, 64, 3, LIMIT, [64])
    add(Case.of("limit inside the first record's frames lets the second in", 256, 0, [b"abc", b"d", b"e"], limit=65),
        H(35, 0xC0, 1, 0) + b"abc" + bytes(29) + H(33, 0xC0, 1, 64) + b"d" + bytes(31) + S(128), 2, 128, 4, LIMIT, [64, 128])
    add(Case.of("too long", 256, 0, [b"abc", b"defgh", b"e"], max_message_length=4),
        H(35, 0xC0, 1, 0) + b"abc" + bytes(29) + S(192), 1, 64, 3, TOO_LONG, [64])
    add(Case.of("the limit is tested before the length", 256, 0, [b"abc", b"defgh"], max_message_length=4, limit=64),
        H(35, 0xC0, 1, 0) + b"abc" + bytes(29) + S(192), 1, 64, 3, LIMIT, [64])
    add(Case("a decreasing offset", 256, 0, b"abcdef", [0, 3, 2, 6]),
        H(35, 0xC0, 1, 0) + b"abc" + bytes(29) + S(192), 1, 64, 3, BAD_RECORD, [64])
    add(Case("an offset past the input", 256, 0, b"abcdef", [0, 3, 7]),
        H(35, 0xC0, 1, 0) + b"abc" + bytes(29) + S(192), 1, 64, 3, BAD_RECORD, [64])
    add(Case("a bad record wins over the limit", 256, 0, b"abcdef", [0, 3, 7], limit=64),
        H(35, 0xC0, 1, 0) + b"abc" + bytes(29) + S(192), 1, 64, 3, BAD_RECORD, [64])
    add(Case.of("no records", 64, 32, []), S(64), 0, 32, 0, END, [])
    return out


HAND_CASES = _hand_cases()

MTUS = (64, 96, 1408)


def edge_lengths(mtu):
    maxp = mtu - HDR
    return [0, 1, 31, 32, 33, maxp - 1, maxp, maxp + 1, 2 * maxp, 2 * maxp + 1]


def random_records(count, seed, mtu=1408, long_every=64):
    """Config-3-style records (a few hundred bytes), one in `long_every` longer than a frame."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(3000, 9000)) if long_every and i % long_every == long_every - 1 else int(rng.integers(180, 420))
        out.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    return out


def exact_block(records, mtu, start=0):
    return start + sum(required(len(r), mtu) for r in records)


def length_filling(space, mtu):
    """The record length whose frames take exactly `space` bytes (the longest such)."""
    maxp = mtu - HDR
    full, r = divmod(space, mtu)
    length = full * maxp + (r - HDR if r else 0)
    assert (r == 0 or r > HDR or full == 0) and r >= (HDR if full == 0 else 0) and required(length, mtu) == space, (space, mtu)
    return length


def shared_cases(tile=16384):
    """The cases the device, the host mirror and the stand-alone host program all run."""
    cases = [c for c, *_ in HAND_CASES]
    hdr = (3, -5, 77, 0x01020304, 1 << 20)
    for mtu in MTUS:
        recs = [rec(n, k) for k, n in enumerate(edge_lengths(mtu))]
        size = exact_block(recs, mtu)
        cases.append(Case.of("lengths mtu %d exact" % mtu, size, 0, recs, mtu=mtu))
        cases.append(Case.of("lengths mtu %d short" % mtu, 96 + size - 32, 96, recs, lead=5, mtu=mtu, header=hdr))
        cases.append(Case.of("lengths mtu %d start at the end" % mtu, 64, 64, recs, mtu=mtu))
    # the second record's frames end exactly at `tile`, the fourth covers more than three tiles
    recs = [rec(100, 1), rec(length_filling(tile - 160, 1408), 2), rec(10, 3), rec(3 * tile, 4), rec(7, 5)]
    cases.append(Case.of("tile edges", exact_block(recs, 1408) + 64, 0, recs, lead=3, header=hdr))
    cases.append(Case.of("trip in a later tile", 2 * tile + 4096, 0, recs, lead=9))
    data, off = pack([rec(5, 1), rec(6, 2), rec(7, 3), rec(8, 4)])
    cases.append(Case("malformed in the middle", 1024, 0, data, [off[0], off[1], off[3], off[2], off[4]]))
    cases.append(Case("first offset past the input", 1024, 0, data, [len(data) + 1, len(data) + 2]))
    cases.append(Case("huge offset", 1024, 0, data, [0, 5, (1 << 64) - 1, 11]))
    return cases


def write_cases(path, cases):
    """The case file of tests/termappend/*: u64 count, then per case u64 {block bytes, start, limit,
    mtu, max_message_length, in bytes, n, appended, next, payload, stop}, i32 {session, stream, term,
    base, version}, the input bytes, rec_off (u64 x n + 1), rec_tail (u64 x appended), the expected
    block (the call runs on a block filled with 0xA5)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for c in cases:
            e = c.expect()
            n = len(c.rec_off) - 1
            f.write(struct.pack("<11Q", c.block_bytes, c.start, NO_LIMIT if c.limit is None else c.limit, c.mtu,
                                MAX_LEN if c.max_message_length is None else c.max_message_length, len(c.data), n,
                                e["appended"], e["next"], e["payload"], e["stop"]))
            version, session, stream, term, base = c.header
            f.write(struct.pack("<5i", session, stream, term, base, version))
            f.write(c.data)
            f.write(np.asarray(c.rec_off, np.uint64).tobytes())
            f.write(np.asarray(e["rec_tail"], np.uint64).tobytes())
            f.write(e["block"])
