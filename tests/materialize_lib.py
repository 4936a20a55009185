"""Hand-built descriptor batches for MATERIALIZE (sbe_materialize_views) at the edges of its copy
kernel (mat_tile in csrc/sbe_codec.hip), with the expected arena from the plain gather
sbe_testlib.oracle_materialize and, per 64-record tile, the classes the tile falls in.

The kernel reads only rec_off, view_off and view_len, so a batch is built from per-record
(view_off[5], view_len[5], record_length) with no encoder or decoder in the way; record bytes are
random printable characters.  One case occupies one 64-record tile (one copy wave); the lanes a case
does not use hold records whose five views are empty.

The classes are arithmetic on the view lengths, a model of the copy wave's round loop: a record
whose written bytes exceed K_MAT_WIN - 16 is copied straight to the arena (direct); the others are
staged, round by round, into a window of K_MAT_WIN bytes that starts at the first unfinished
record's arena offset rounded down to 16 bytes of the arena's address, and a round takes every
unfinished record that ends inside the window.  K_MAT_WIN mirrors SBE_MAT_WIN (kMatWin) of
csrc/sbe_codec.hip: if that is ever rebuilt to another value, K_MAT_WIN and the B values of family W
must move with it, or these cases no longer sit on the boundary they are meant to pin
(tests/test_materialize_lib.py compares the two).

  has_direct        some record of the tile is copied direct
  direct_between    a round of a loop that does not stop at direct records would span a direct
                    record's arena range: a non-empty staged record before and after it in one
                    window (the stores of such a round would cover the direct record's bytes)
  spans_two_rounds  the staged records of the tile need more than one window
"""
from dataclasses import dataclass, field

import numpy as np

import sbe_testlib as T

K_MAT_WIN = 16384            # SBE_MAT_WIN of csrc/sbe_codec.hip
DIRECT_OVER = K_MAT_WIN - 16  # written bytes above this: copied direct
TILE = 64                    # records of one copy wave (kMatTile)
SCAN_ROUND = 1024 * 1024     # records one loop round of mat_scan_blocks covers (kMatBlk block sums of kMatBlk)
SHIFTS = (0, 1, 8, 15)       # bytes the arena tensor is advanced by

EMPTY = ((0, 0, 0, 0, 0), (0, 0, 0, 0, 0), 4)  # a record with five empty views

W_A = (0, 1, 7, 15, 16, 17)
W_C = (0, 1, 8, 15, 16)
W_B = (16352, 16367, 16368, 16369, 16370, 16376, 16382, 16383, 16384, 16385, 16400, 32768, 65534)
W_LANES = ((0, 1, 2), (61, 62, 63), (10, 30, 50))


@dataclass
class Batch:
    data: np.ndarray       # uint8: the records back to back
    rec_off: np.ndarray    # uint64 [n + 1]
    view_off: np.ndarray   # uint32 [n, 5]
    view_len: np.ndarray   # uint32 [n, 5]
    exp: np.ndarray        # uint8: oracle_materialize's arena
    exp_off: np.ndarray    # uint64 [5 n + 1]
    names: list = field(default_factory=list)  # one per tile

    @property
    def n(self):
        return self.rec_off.size - 1

    @property
    def tiles(self):
        return (self.n + TILE - 1) // TILE

    @property
    def dec(self):
        return {"view_off": self.view_off, "view_len": self.view_len}


# ------------------------------------------------------------------------------------------
# records
# ------------------------------------------------------------------------------------------
def make_rec(lens, rng, order="inc", head=None, tail=None):
    """A record holding five views of the given lengths: laid out in source order `order` ("inc":
    view 0 first, "dec": view 4 first, "shuf": a random order) behind `head` bytes, 0..2 bytes
    between views, `tail` bytes after the last (0: that view ends exactly at the record's end)."""
    lens = [int(x) for x in lens]
    assert len(lens) == 5
    perm = {"inc": [0, 1, 2, 3, 4], "dec": [4, 3, 2, 1, 0]}.get(order)
    if perm is None:
        perm = [int(x) for x in rng.permutation(5)]
    pos = int(rng.integers(0, 9)) if head is None else head
    off = [0] * 5
    for k in perm:
        off[k] = pos
        pos += lens[k] + int(rng.integers(0, 3))
    end = max(off[k] + lens[k] for k in range(5))
    rl = end + (int(rng.integers(0, 20)) if tail is None else tail)
    return tuple(off), tuple(lens), max(rl, 1)


def split_five(total, slot, rng):
    """`total` bytes as four views of 1..15 bytes and the remainder in view `slot`."""
    lens = [int(x) for x in rng.integers(1, 16, 5)]
    lens[slot] = 0
    lens[slot] = total - sum(lens)
    assert lens[slot] > 0
    return lens


def tile_of(lanes):
    """A 64-record tile from {lane: record}; the other lanes hold empty records."""
    t = [EMPTY] * TILE
    for lane, r in lanes.items():
        assert 0 <= lane < TILE
        t[lane] = r
    return t


def build(tiles, seed, names=None):
    """A Batch of the given tiles (lists of up to 64 records; a short tile is filled with empty ones)."""
    rng = np.random.default_rng(seed)
    recs = []
    for t in tiles:
        assert len(t) <= TILE
        recs.extend(list(t) + [EMPTY] * (TILE - len(t)))
    n = len(recs)
    vo = np.array([r[0] for r in recs], np.uint32).reshape(n, 5)
    vl = np.array([r[1] for r in recs], np.uint32).reshape(n, 5)
    rl = np.array([r[2] for r in recs], np.uint64)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(rl)
    data = rng.integers(32, 127, int(off[-1]), dtype=np.uint8)
    exp, exp_off = T.oracle_materialize(data, off, {"view_off": vo, "view_len": vl})
    return Batch(data, off, vo, vl, exp, exp_off, list(names) if names is not None else [""] * len(tiles))


# ------------------------------------------------------------------------------------------
# the round model
# ------------------------------------------------------------------------------------------
def written(at, cap):
    """(o, fit) of a record with arena offsets at[0..5]: its views that end within cap are written."""
    fit = at[0]
    for k in range(5):
        if at[k + 1] <= cap:
            fit = at[k + 1]
    return at[0], fit


def rounds(o, fit, shift, bounded):
    """The window rounds of one tile: [(start, cend, staged lanes)].  o / fit: per lane, the arena
    offsets of the record's first byte and of the end of its written bytes; shift: the arena's
    address mod 16.  bounded: a round ends at the first direct record at or after its start."""
    m = len(o)
    direct = [fit[i] - o[i] > DIRECT_OVER for i in range(m)]
    done = [fit[i] == o[i] or direct[i] for i in range(m)]
    out = []
    while not all(done):
        start = min(o[i] for i in range(m) if not done[i])
        wbase = start - ((shift + start) & 15)
        bound = None
        if bounded:
            d = [o[i] for i in range(m) if direct[i] and o[i] >= start]
            bound = min(d) if d else None
        staged = [i for i in range(m) if not done[i] and fit[i] - wbase <= K_MAT_WIN and
                  (bound is None or fit[i] <= bound)]
        assert staged, "a round finishes at least the record at its start"
        out.append((start, max(fit[i] for i in staged), staged))
        for i in staged:
            done[i] = True
    return out


def tile_classes(o, fit, shift):
    """(classes, clobbered): the set of classes of one tile, and the bytes of direct records that a
    round loop which does not stop at direct records would store over."""
    m = len(o)
    direct = [i for i in range(m) if fit[i] - o[i] > DIRECT_OVER]
    cls = set()
    if direct:
        cls.add("has_direct")
    free = rounds(o, fit, shift, bounded=False)
    clobbered = 0
    for start, cend, _ in free:
        for i in direct:
            clobbered += max(0, min(fit[i], cend) - max(o[i], start))
    if clobbered:
        cls.add("direct_between")
    if len(free) > 1:
        cls.add("spans_two_rounds")
    return cls, clobbered


def classes(b: Batch, shift=0, cap=None):
    """Per tile of the batch: (classes, clobbered bytes, the tile's own arena offset)."""
    cap = int(b.exp_off[-1]) if cap is None else cap
    at = b.exp_off.astype(np.int64).tolist()
    out = []
    for t in range(b.tiles):
        o, fit = [], []
        for i in range(t * TILE, min((t + 1) * TILE, b.n)):
            oo, ff = written(at[5 * i: 5 * i + 6], cap)
            o.append(oo)
            fit.append(ff)
        cls, clob = tile_classes(o, fit, shift)
        out.append((cls, clob, at[5 * t * TILE]))
    return out


def lens_classes(lens, base=0, shift=0):
    """tile_classes of a tile whose records carry `lens` view bytes each, from arena offset base."""
    o, fit, p = [], [], base
    for x in lens:
        o.append(p)
        p += x
        fit.append(p)
    return tile_classes(o, fit, shift)


def span_misalignment(b: Batch, t, shift=0):
    """(arena address of tile t's first non-empty staged record) mod 16."""
    at = b.exp_off.astype(np.int64)
    for i in range(t * TILE, min((t + 1) * TILE, b.n)):
        sz = int(at[5 * i + 5] - at[5 * i])
        if 0 < sz <= DIRECT_OVER:
            return int(at[5 * i] + shift) & 15
    return 0


# ------------------------------------------------------------------------------------------
# family W: the window / direct boundary
# ------------------------------------------------------------------------------------------
def _small(x, rng, j):
    """A record of x view bytes: one view, or (every other one, from 5 bytes up) spread over the slots."""
    if x >= 5 and j % 2:
        lens = [1, 1, 1, 1, x - 4]
        rng.shuffle(lens)
        return make_rec(lens, rng, order="shuf")
    lens = [0] * 5
    lens[j % 5] = x
    return make_rec(lens, rng)


def _big(B, five, slot, rng, j):
    if five:
        return make_rec(split_five(B, slot, rng), rng, order=("inc", "dec", "shuf")[j % 3],
                        tail=(0 if j % 4 == 0 else None))
    lens = [0] * 5
    lens[slot] = B
    return make_rec(lens, rng, tail=(0 if j % 4 == 1 else None))


def family_w(seed=0xA7E1):
    """Triples a | B | c at three lane placements: every B with every placement and every (a, c);
    the view layout of B (one view, or four views of 1..15 bytes and the remainder, in every slot)
    rotates over the product (the B of 16369..16382 bytes, which can sit inside one window span, take
    both layouts everywhere), and the two largest B keep a third of their (a, c) pairs."""
    rng = np.random.default_rng(seed)
    tiles, names = [], []
    j = 0
    for B in W_B:
        for ia, a in enumerate(W_A):
            for ic, c in enumerate(W_C):
                if B >= 32768 and (ia + ic) % 3:
                    continue
                for il, lanes in enumerate(W_LANES):
                    # both layouts where a direct record can sit inside one window span
                    forms = (False, True) if DIRECT_OVER < B < K_MAT_WIN - 1 else ((ia + ic + il) % 2 == 1,)
                    for five in forms:
                        slot = (ia + 2 * ic + il) % 5
                        tiles.append(tile_of({lanes[0]: _small(a, rng, j), lanes[1]: _big(B, five, slot, rng, j),
                                              lanes[2]: _small(c, rng, j + 1)}))
                        names.append(f"W a={a} B={B}{'/5v' if five else ''} c={c} lanes={lanes}")
                        j += 1
    # the a side as several records; zero-length records inside the span
    for B in (16368, 16369, 16370, 16376, 16382, 16383):
        for c in (1, 8):
            for first in (0, 20, 59):
                t = {first + k: _small(2, rng, j + k) for k in range(3)}
                t[first + 3] = _big(B, j % 2 == 0, j % 5, rng, j)
                t[first + 4] = _small(c, rng, j)
                tiles.append(tile_of(t))
                names.append(f"W a=3x2 B={B} c={c} lanes={first}..{first + 4}")
                j += 1
    # the same boundary with the tile's own arena offset chosen: a tile of one record brings the
    # running total to r mod 16 first, so the span starts r bytes off 16-byte alignment
    total = sum(sum(rec[1]) for t in tiles for rec in t)
    for B in (16369, 16370, 16376, 16382):
        for r in (0, 1, 2, 5, 15):
            for a, c in ((1, 1), (1, 8), (7, 1), (7, 8)):
                pad = (r - total) % 16
                if pad:
                    tiles.append(tile_of({j % TILE: _small(pad, rng, j)}))
                    names.append(f"W pad {pad}")
                lanes = W_LANES[j % 3]
                tiles.append(tile_of({lanes[0]: _small(a, rng, j), lanes[1]: _big(B, j % 2 == 1, j % 5, rng, j),
                                      lanes[2]: _small(c, rng, j + 1)}))
                names.append(f"W at {r} mod 16: a={a} B={B} c={c} lanes={lanes}")
                total += pad + a + B + c
                j += 1
    # two direct records in one tile: apart (a small record between them) and adjacent
    for B1 in (16369, 16370, 16382, 32768):
        for B2 in (16369, 16376, 16385):
            for mid in (None, 0, 1, 5):
                t = {3: _small(1 + j % 3, rng, j), 4: _big(B1, j % 2 == 1, j % 5, rng, j)}
                lane = 5
                if mid is not None:
                    t[lane] = _small(mid, rng, j)
                    lane += 1
                t[lane] = _big(B2, j % 2 == 0, (j + 2) % 5, rng, j + 1)
                t[lane + 1] = _small(1 + j % 4, rng, j)
                tiles.append(tile_of(t))
                names.append(f"W two direct B={B1},{B2} mid={mid}")
                j += 1
    return build(tiles, seed ^ 0x55, names)


# ------------------------------------------------------------------------------------------
# family S: short views and small records
# ------------------------------------------------------------------------------------------
def family_s(seed=0x5A11):
    """Records of 1..40 bytes carrying every (offset, length 0..15) view that fits in them (views
    that end at the record's end included), five to a record in random, hence overlapping and
    unordered, source positions; a third of them again with the views in non-increasing source
    order; records of 17..64 bytes that mix views of 0..15 and of 16..48 bytes; and tiles of ~1 KiB
    records among the short ones, whose staged bytes need two windows."""
    rng = np.random.default_rng(seed)
    recs = []
    for rl in range(1, 41):
        views = [(o, ln) for o in range(rl + 1) for ln in range(0, min(15, rl - o) + 1)]
        rng.shuffle(views)
        while len(views) % 5:
            views.append((rl, 0))
        for g in range(0, len(views), 5):
            grp = views[g: g + 5]
            recs.append((tuple(o for o, _ in grp), tuple(ln for _, ln in grp), rl))
            if (g // 5) % 3 == 0:  # the same views in non-increasing source order
                grp = sorted(grp, key=lambda v: -v[0])
                recs.append((tuple(o for o, _ in grp), tuple(ln for _, ln in grp), rl))
    for rl in range(17, 65):
        for rep in range(30):
            offs, lens = [], []
            for k in range(5):
                ln = int(rng.integers(16, min(48, rl) + 1)) if (k + rep) % 2 else int(rng.integers(0, 16))
                ln = min(ln, rl)
                o = rl - ln if (k + rep) % 5 == 0 else int(rng.integers(0, rl - ln + 1))
                offs.append(o)
                lens.append(ln)
            recs.append((tuple(offs), tuple(lens), rl))
    order = rng.permutation(len(recs))
    recs = [recs[i] for i in order]
    tiles = [recs[g: g + TILE] for g in range(0, len(recs), TILE)]
    names = [f"S short {g}" for g in range(len(tiles))]
    for g in range(24):  # 20 records of ~1 KiB among 44 short ones: more than one window of staged bytes
        t = [recs[(g * 44 + k) % len(recs)] for k in range(44)]
        for k in range(20):
            lens = [int(x) for x in rng.integers(0, 16, 5)]
            lens[(g + k) % 5] = int(rng.integers(990, 1100))
            t.insert(int(rng.integers(0, len(t) + 1)), make_rec(lens, rng, order=("inc", "dec", "shuf")[k % 3]))
        tiles.append(t)
        names.append(f"S two rounds {g}")
    return build(tiles, seed ^ 0x55, names)


# ------------------------------------------------------------------------------------------
# family C: capacity cuts over W tiles
# ------------------------------------------------------------------------------------------
C_FORMS = (
    ("one view 16368 (staged)", (0, 0, 16368, 0, 0)),
    ("one view 16370", (16370, 0, 0, 0, 0)),
    ("one view 65534", (0, 0, 0, 0, 65534)),
    ("five views, direct at every cut from view 0 on", (16370, 5, 5, 5, 5)),      # truncated sizes stay over 16368
    ("five views, direct in full, staged when cut", (8000, 8000, 300, 60, 40)),  # 16400 in full, 16000..16360 cut
    ("five views 16386", (3, 7, 16360, 1, 15)),
)


def family_c(seed=0xCA9):
    """[(Batch, index of the B record, [capacities])]: an a | B | c tile behind a tile of a few small
    records (so the tile's own arena offset is not a multiple of 16; every other case has none),
    cut inside B's first view, at every arena_off boundary of B, at B's end and one byte either
    side, inside c, and at 0."""
    rng = np.random.default_rng(seed)
    out = []
    for f, (name, lens) in enumerate(C_FORMS):
        for v, lanes in enumerate(((0, 1, 2), (10, 30, 50))):
            a, c = (7, 8) if v == 0 else (1, 3)
            w = tile_of({lanes[0]: _small(a, rng, f), lanes[1]: make_rec(lens, rng, order=("inc", "shuf")[v]),
                         lanes[2]: _small(c, rng, f + 1)})
            pre = (f + v) % 2 == 0
            tiles = ([[_small(7, rng, k) for k in range(5)]] if pre else []) + [w]
            b = build(tiles, seed + 16 * f + v, (["C prefix"] if pre else []) + [f"C {name} lanes={lanes}"])
            i = (TILE if pre else 0) + lanes[1]
            at = b.exp_off[5 * i: 5 * i + 6].astype(np.int64).tolist()
            first = next(k for k in range(5) if lens[k])
            caps = {0, at[first] + 1, at[first] + lens[first] // 2, at[5] - 1, at[5], at[5] + 1, at[5] + c // 2 + 1,
                    int(b.exp_off[-1])}
            caps.update(at[1:5])
            out.append((b, i, sorted(x for x in caps if 0 <= x <= int(b.exp_off[-1]))))
    return out


# ------------------------------------------------------------------------------------------
# family N: the carry of the block-sum scan
# ------------------------------------------------------------------------------------------
N_SIZES = (SCAN_ROUND + 1, SCAN_ROUND + 2048 + 37)


def family_n(n):
    """n records of 4 bytes, record i with one view of i % 5 bytes in slot (i // 5) % 5: more
    records than one round of the block-sum scan takes, so the scan's carry is used."""
    rng = np.random.default_rng(n)
    i = np.arange(n)
    vl = np.zeros((n, 5), np.uint32)
    vo = np.zeros((n, 5), np.uint32)
    slot = (i // 5) % 5
    vl[i, slot] = i % 5
    vo[i, slot] = (4 - i % 5) * ((i // 25) % 2)  # at the record's start, or ending at its end
    off = (4 * np.arange(n + 1)).astype(np.uint64)
    data = rng.integers(32, 127, 4 * n, dtype=np.uint8)
    exp, exp_off = T.oracle_materialize(data, off, {"view_off": vo, "view_len": vl})
    return Batch(data, off, vo, vl, exp, exp_off, [])
