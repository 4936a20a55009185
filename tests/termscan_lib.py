"""Aeron term-buffer framing for the tests of sbe_term_scan: the walk restated in Python, a block
builder, hand-written cases with their expected tables spelled out, the blocks the GPU and host
tests share, and the case file the C++ programs of tests/term read.

The frame layer is third-party Aeron (absent from the reference tree), so the walk is restated from
the data-frame layout and the TermReader::read loop, not compiled: the 32-byte little-endian header
  [0] i32 frame_length  [4] i8 version  [5] u8 flags  [6] u16 type  [8] i32 term_offset
  [12] i32 session_id  [16] i32 stream_id  [20] i32 term_id  [24] i64 reserved_value
on a 32-byte boundary, the next frame align(frame_length, 32) bytes on."""
import os
import struct

import numpy as np

import sbe_testlib as T

DIR = os.path.join(T.ROOT, "tests", "term")
END, LIMIT, UNCOMMITTED, SHORT, PARTIAL = range(5)
HDR = 32
BEGIN, ENDF = 0x80, 0x40


def align(n):
    return (n + 31) & ~31


def walk(block, start=0, limit=None):
    """The poll of one image over block[start:], restated.  Returns a dict of the tables
    sbe_term_scan writes: frag_src, flags, frag_off (offsets of the payloads laid back to back),
    payload (those bytes), fragments, next, stop."""
    block = bytes(block)
    n = len(block)
    if limit is None:
        limit = 1 << 62
    offset, src, flags, lens = start, [], [], []
    stop = None
    while len(src) < limit and offset < n:
        (length,) = struct.unpack_from("<i", block, offset)
        if length <= 0:
            stop = UNCOMMITTED
            break
        if length < HDR:
            stop = SHORT
            break
        if offset + align(length) > n:
            stop = PARTIAL
            break
        frame = offset
        offset += align(length)
        if struct.unpack_from("<H", block, frame + 6)[0] != 0:
            src.append(frame)
            flags.append(block[frame + 5])
            lens.append(length - HDR)
    if stop is None:
        stop = LIMIT if len(src) == limit else END
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    payload = b"".join(block[s + HDR: s + HDR + k] for s, k in zip(src, lens))
    return dict(frag_src=src, flags=flags, frag_off=off, payload=payload, fragments=len(src), next=offset,
                stop=stop)


def header(length, flags=BEGIN | ENDF, ftype=1, term_offset=0):
    return struct.pack("<iBBHiiiiq", length, 1, flags, ftype, term_offset, 7, 1001, 3, 0)


class Block:
    """Frames appended one after another; raw bytes may be planted anywhere afterwards."""

    def __init__(self):
        self.b = bytearray()

    def __len__(self):
        return len(self.b)

    def frame(self, payload=b"", flags=BEGIN | ENDF, ftype=1, length=None):
        """A frame with `payload`; `length` overrides the frame_length written (the frame still
        occupies align(32 + len(payload)) bytes of the block).  Returns its offset."""
        at = len(self.b)
        n = HDR + len(payload)
        self.b += header(n if length is None else length, flags, ftype, at) + bytes(payload)
        self.b += bytes(align(n) - n)
        return at

    def pad(self, total):
        """A padding frame (type 0) that occupies `total` bytes (a multiple of 32)."""
        assert total % 32 == 0 and total >= 32
        return self.frame(bytes(total - HDR), 0, 0)

    def pad_to(self, offset):
        if offset > len(self.b):
            self.pad(offset - len(self.b))
        assert len(self.b) == offset, (len(self.b), offset)

    def raw(self, data):
        at = len(self.b)
        self.b += bytes(data)
        return at

    def plant(self, offset, data):
        self.b[offset: offset + len(data)] = bytes(data)

    def zeros_to(self, offset):
        self.b += bytes(offset - len(self.b))

    def bytes(self):
        assert len(self.b) % 32 == 0
        return bytes(self.b)


def decoys(nbytes, length_of):
    """A payload of nbytes (a multiple of 32) that is a well-formed header at every 32-byte
    position: slot j's frame_length is length_of(j), its type 1 (a data frame)."""
    assert nbytes % 32 == 0
    return b"".join(header(length_of(j), BEGIN | ENDF, 1, 0) for j in range(nbytes // 32))


# ---- hand cases: (name, block, start, limit, expected) with the tables written out ----
def _hand_cases():
    cases = []

    def add(name, blk, start, limit, src, flags, off, nxt, stop):
        cases.append((name, blk, start, limit,
                      dict(frag_src=src, flags=flags, frag_off=off, fragments=len(src), next=nxt, stop=stop)))

    add("empty block", b"", 0, None, [], [], [0], 0, END)
    b = Block()
    b.frame(b"abc")
    add("start at the end", b.bytes(), 64, None, [], [], [0], 64, END)
    add("limit 0", b.bytes(), 0, 0, [], [], [0], 0, LIMIT)
    add("limit 0 at the end", b.bytes(), 64, 0, [], [], [0], 64, LIMIT)
    add("one frame", b.bytes(), 0, None, [0], [0xC0], [0, 3], 64, END)
    add("one frame, limit 1", b.bytes(), 0, 1, [0], [0xC0], [0, 3], 64, LIMIT)
    add("length 0", bytes(64), 0, None, [], [], [0], 0, UNCOMMITTED)
    add("negative length", header(-64) + bytes(32), 0, None, [], [], [0], 0, UNCOMMITTED)
    add("a 32-byte frame is an empty fragment", header(32, 0x80), 0, None, [0], [0x80], [0, 0], 32, END)
    b = Block()
    b.pad(96)
    add("padding only", b.bytes(), 0, None, [], [], [0], 96, END)
    b = Block()
    b.frame(b"x" * 33, 0x80)   # 0: 65 bytes -> 96
    b.pad(64)                  # 96
    b.frame(b"y" * 32, 0x40)   # 160: 64 bytes
    b.frame(b"", 0xC0)         # 224
    add("chain with padding", b.bytes(), 0, None, [0, 160, 224], [0x80, 0x40, 0xC0], [0, 33, 65, 65], 256, END)
    add("padding before the limit-th fragment is consumed", b.bytes(), 0, 2, [0, 160], [0x80, 0x40], [0, 33, 65],
        224, LIMIT)
    add("padding after the limit-th fragment is not", b.bytes(), 0, 1, [0], [0x80], [0, 33], 96, LIMIT)
    add("start inside", b.bytes(), 160, None, [160, 224], [0x40, 0xC0], [0, 32, 32], 256, END)
    for length, stop in ((1, SHORT), (31, SHORT), (65, PARTIAL), (0x7fffffff, PARTIAL), (0, UNCOMMITTED)):
        b = Block()
        b.frame(b"ab")
        b.raw(header(length) + bytes(32))
        add("stop %d after one frame (length %d)" % (stop, length), b.bytes(), 0, None, [0], [0xC0], [0, 2], 64, stop)
    # a payload that looks like headers: slot 1 (offset 32) says "32-byte frame", and is not one
    b = Block()
    b.frame(decoys(64, lambda j: 32), 0xC0)
    b.frame(b"z", 0x80)
    add("decoy headers in a payload", b.bytes(), 0, None, [0, 96], [0xC0, 0x80], [0, 64, 65], 160, END)
    return cases


HAND_CASES = _hand_cases()


# ---- blocks shared by the GPU and host tests ----
def lengths_block():
    """Payload lengths 1, 31, 32, 33, 1376 and 1377 in one chain."""
    b = Block()
    for k, n in enumerate((1, 31, 32, 33, 1376, 1377)):
        b.frame(bytes((7 * k + j) & 0xff for j in range(n)), (0x80, 0x00, 0x40, 0xC0)[k % 4])
    return b.bytes()


def decoy_block():
    """Payloads filled with well-formed headers at every 32-byte position, of every kind."""
    b = Block()
    kinds = [
        lambda j: 32,           # the successor is the next decoy
        lambda j: 64,
        lambda j: 1 << 20,      # points past the block
        lambda j: 0x7fffffff,
        lambda j: 0,
        lambda j: -32,
        lambda j: 1 + j % 31,   # 1..31
    ]
    real = []
    for k, kind in enumerate(kinds):
        size = 32 * (3 + 5 * k)
        # decoys whose successor lands exactly on the next real frame: the last slot says 32
        real.append(b.frame(decoys(size, kind), (0xC0, 0x80, 0x40)[k % 3]))
        real.append(b.frame(b"r%d" % k, 0xC0))
    # one whose decoy successor lands on a real frame further on
    at = len(b)
    b.frame(decoys(96, lambda j: 32 * (3 - j) + 32 * 2), 0xC0)  # every decoy points at the frame after next
    real.append(at)
    real.append(b.frame(b"after", 0x80))
    real.append(b.frame(b"target", 0x40))
    return b.bytes(), real


def tile_block(tile):
    """Frames placed against tile edges (tile = sbe_term_scan_tile()): one that ends exactly at
    the first edge, one that straddles the second, a padding frame over more than two whole tiles,
    a frame in the last slot of a tile, data afterwards."""
    b = Block()
    b.frame(b"a" * 100, 0x80)
    b.frame(bytes(j & 0xff for j in range(tile - len(b) - HDR)), 0x40)      # ends exactly at tile
    assert len(b) == tile
    b.frame(b"b" * 40, 0xC0)
    b.pad_to(2 * tile - 64)
    b.frame(bytes((3 * j) & 0xff for j in range(200)), 0xC0)                # straddles 2 * tile
    b.frame(b"c", 0x80)
    b.pad_to(7 * tile - 32)                                                 # covers tiles 3, 4 and 5 whole
    b.frame(b"d" * 5, 0x00)                                                 # tile 6 is entered in its last slot
    b.pad_to(8 * tile - 32)
    b.frame(b"", 0x40)                                                      # a frame that is the last slot of a tile
    b.frame(b"e" * 64, 0xC0)
    b.frame(b"g" * 9, 0xC0)
    return b.bytes()


def stop_blocks(tile):
    """(name, block) for SHORT, PARTIAL and UNCOMMITTED stops in the first tile and in a later one."""
    out = []
    for where in ("first", "later"):
        for name, length in (("short", 17), ("partial", 4096), ("partial-max", 0x7fffffff), ("uncommitted", 0),
                             ("negative", -1)):
            b = Block()
            b.frame(b"head", 0xC0)
            if where == "later":
                b.frame(b"x" * 300, 0xC0)
                b.pad_to(tile + 32 * 5)
                b.frame(b"y" * 33, 0xC0)
            b.raw(header(length) + bytes(32 * 3))
            b.raw(header(64) + bytes(32))  # a well-formed frame behind the stop: never reached
            out.append(("%s-%s" % (name, where), b.bytes()))
    return out


def dense_blocks(tile):
    """(name, block) of tiles packed with frames: chains of up to tile / 32 - 1 steps inside one
    tile, past the 512 steps the top doubling level reaches on its own.  Only 32-byte data frames
    (empty fragments), only 32-byte padding frames, 32-byte frames of both kinds mixed, and a mix
    with 64-byte frames; three tiles and a bit each, so that the last tile is part full."""
    slots = 3 * (tile // 32) + 37
    rng = np.random.default_rng(0xDE45)
    out = []
    b = Block()
    for j in range(slots):
        b.frame(b"", (0xC0, 0x80, 0x00, 0x40)[j % 4])
    out.append(("data32", b.bytes()))
    b = Block()
    for j in range(slots):
        b.pad(32)
    out.append(("pad32", b.bytes()))
    b = Block()
    for j in range(slots):
        if rng.random() < 0.3:
            b.pad(32)
        else:
            b.frame(b"", int(rng.choice([0xC0, 0x80, 0x00, 0x40])))
    out.append(("mixed32", b.bytes()))
    b = Block()
    while len(b) < 32 * slots:
        r = rng.random()
        if r < 0.15:
            b.pad(32 if rng.random() < 0.7 else 64)
        elif r < 0.75:
            b.frame(b"", int(rng.choice([0xC0, 0x80, 0x00, 0x40])))
        else:
            b.frame(rng.integers(0, 256, int(rng.integers(1, 33)), dtype=np.uint8).tobytes(), 0xC0)
    out.append(("mixed64", b.bytes()))
    # decoys only, the same lengths: every slot says 32 (or 64), whichever the walk lands on
    lens = rng.choice([32, 64], slots, p=[.85, .15])
    lens[-1] = 32
    out.append(("decoy32", decoys(32 * slots, lambda j: int(lens[j]))))
    return out


def dense_calls(tile):
    """(start, limit) pairs for a dense block: start at 0 and mid-tile, limits in the second half
    of a tile and in the last tile."""
    n = tile // 32
    return [(0, None), (32 * (n // 2 + 3), None), (32 * (n + 700), None), (0, n // 2 + 200), (0, n - 1), (0, n), (0, n + 1),
            (0, 2 * n + 600), (0, 3 * n + 5), (32 * 5, 3 * n), (32 * (n - 1), 700)]


def random_block(slots, seed, p_decoy=0.25, p_pad=0.15, max_payload=1376):
    """A fixed-seed block of `slots` slots: data frames with random payloads (a share of them filled
    with decoy headers), padding frames in between, the tail closed with a padding frame."""
    rng = np.random.default_rng(seed)
    total = 32 * slots
    b = Block()
    while total - len(b) > align(HDR + max_payload) + 32:
        r = rng.random()
        if r < p_pad:
            b.pad(32 * int(rng.integers(1, 40)))
            continue
        n = int(rng.integers(0, max_payload + 1))
        fl = int(rng.choice([0xC0, 0x80, 0x00, 0x40]))
        if rng.random() < p_decoy and n >= 32:
            lens = rng.choice([32, 64, 96, 1408, 0, -5, 7, 31, 1 << 24, 0x7fffffff], n // 32)
            pay = decoys(32 * (n // 32), lambda j: int(lens[j])) + bytes(n % 32)
        else:
            pay = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        b.frame(pay, fl)
    b.pad_to(total)
    return b.bytes()


def framed_records(records, mtu=1376, pad_every=0):
    """Records (bytes) framed as a publication would: one BEGIN|END frame each, or BEGIN / middle /
    END frames of at most `mtu` payload bytes.  Returns the block."""
    b = Block()
    for i, rec in enumerate(records):
        parts = [rec[k: k + mtu] for k in range(0, len(rec), mtu)] or [b""]
        for t, p in enumerate(parts):
            fl = (BEGIN if t == 0 else 0) | (ENDF if t == len(parts) - 1 else 0)
            b.frame(p, fl)
        if pad_every and i % pad_every == pad_every - 1:
            b.pad(64)
    return b.bytes()


def write_cases(path, cases):
    """The case file of tests/term/*: u64 count, then per case u64 block bytes, start, limit,
    fragments, next, stop; the block; frag_off (u64 x fragments + 1), frag_src (u32), flags (u8).
    cases: (block, start, limit) — the expectation is walk()'s."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for blk, start, limit in cases:
            w = walk(blk, start, limit)
            lim = (1 << 62) if limit is None else limit
            f.write(struct.pack("<QQQQQQ", len(blk), start, lim, w["fragments"], w["next"], w["stop"]))
            f.write(blk)
            f.write(np.asarray(w["frag_off"], np.uint64).tobytes())
            f.write(np.asarray(w["frag_src"], np.uint32).tobytes())
            f.write(np.asarray(w["flags"], np.uint8).tobytes())


def adversarial_cases(tile=32768):
    """Every malformed or awkward block above, as (block, start, limit)."""
    cases = [(blk, start, limit) for _, blk, start, limit, _ in HAND_CASES]
    cases.append((lengths_block(), 0, None))
    cases.append((decoy_block()[0], 0, None))
    cases.append((decoy_block()[0], 0, 5))
    tb = tile_block(tile)
    cases += [(tb, 0, None), (tb, tile + 32, None), (tb, 0, 3)]
    cases += [(blk, 0, None) for _, blk in stop_blocks(tile)]
    for _, blk in dense_blocks(tile):
        cases += [(blk, start, limit) for start, limit in dense_calls(tile)]
    rb = random_block(4096, 11)
    cases += [(rb, 0, None), (rb, 0, 100)]
    # headers only: every slot of the block is a decoy of some kind, the chain follows what they say
    rng = np.random.default_rng(3)
    lens = rng.choice([32, 64, 96, 0, -1, 5, 1 << 30, 0x7fffffff, 320], 512, p=[.4, .2, .1, .02, .02, .02, .02, .02, .2])
    cases.append((decoys(32 * 512, lambda j: int(lens[j])), 0, None))
    return cases
