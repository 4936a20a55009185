"""Helpers of test_gpu_second_trip.py and test_gpu_far_input.py: batches large enough that the
size-gated loops of the kernels take their second trip, and how their expected outputs are put
together without a Python loop over the records.

Thresholds.  The single-workgroup "scan of the block sums" launches and the fixed-grid kernels
loop once below a size that follows from a few constants of the sources.  constants() reads them
from the sources, trips() derives from them how often each loop runs at the sizes the tests use,
and tests/test_bigbatch_lib.py asserts that every loop runs twice and that its last trip is
partial: a change of a constant fails that test instead of turning the GPU tests back into
one-trip runs.

The pool method.  Where a record's output does not depend on its position, a batch of n records is
n draws (with replacement, not periodic: the block sums differ from block to block) from a pool of
at most 4096 distinct records.  The oracle runs on the pool; assemble() gathers the batch's input
and its expected stream and offsets from the pool's.  It is plain tensor arithmetic, works on CPU
and device tensors alike, and test_bigbatch_lib.py holds it to the oracle run on a whole batch."""
import os
import re
import struct

import numpy as np
import torch

import report_lib as R
import sbe_testlib as T
import termappend_lib as TA
import termscan_lib as TS

CSRC = os.path.join(T.PKG, "csrc")
N = (1 << 20) + 1025          # the batch size of the second-trip tests unless stated otherwise
N_FRAG_B = (1 << 20) + 2561   # reassembly stream (B): scan blocks 1024 and 1025 whole, 1026 partial
N_COMMIT = (1 << 19) + 257    # commit emit: the second of its two scanned arrays crosses a trip
N_LAT = 2_097_152 + 4097      # latency samples
LAT_CAPACITY = 1 << 22
INF_BIG, INF_SMALL = 1 << 20, 1 << 19  # inflight table capacities
POOL = 4096                   # most distinct records of a pool

_SOURCES = {"sbe_codec.hip": ("SBE_FS_PER", "kFsThreads", "kMatBlk", "SBE_FC_MAXB", "kFragGroup"),
            "order_json.hpp": ("kBlock", "kScanThreads"),
            "delivery_report.hpp": ("kDrBlk", "kDrPer", "kDrSortBlocks", "kDrListBlocks"),
            "inflight.hpp": ("kInfRehashBlocks", "kInfBlk")}


def constants():
    """The constants the thresholds follow from, read from csrc/ (as contract_lib.frag_scan_block
    reads kFsBlk), and the relations between them that the derivations below rely on."""
    c = {}
    src = {}
    for name, names in _SOURCES.items():
        with open(os.path.join(CSRC, name)) as f:
            src[name] = f.read()
        for k in names:
            m = re.search(r"(?:#define\s+%s\s+|\b%s\s*=\s*)(\d+)\b" % (k, k), src[name])
            assert m, f"{k} not found in {name}"
            c[k] = int(m.group(1))
    hip = src["sbe_codec.hip"]
    assert re.search(r"kFsBlk = kFsPer \* kFsThreads", hip) and re.search(r"kFsPer = SBE_FS_PER", hip)
    assert re.search(r"c0 < nb; c0 \+= kFsBlk", hip)            # frag_scan_blocks_body: kFsBlk aggregates a trip
    assert re.search(r"c0 < nb; c0 \+= kMatBlk", hip)           # mat_scan_blocks
    assert re.search(r"\(n \+ 1 \+ 4 \* kFragGroup - 1\) / \(4 \* kFragGroup\)", hip)  # frag_copy: four waves a block
    assert re.search(r"2 \* \(nblk \+ 1\)\)", hip)              # commit_launches: two arrays scanned as one
    with open(os.path.join(CSRC, "term_append.hpp")) as f:
        ta = f.read()
    assert re.search(r"kTaBlk = kMatBlk", ta) and re.search(r"c0 < nb; c0 \+= kTaBlk", ta)
    assert re.search(r"nb = \(n \+ 1 \+ kTaBlk - 1\) / kTaBlk", hip)
    assert re.search(r"c0 < m; c0 \+= 4 \* kScanThreads", src["order_json.hpp"])
    assert re.search(r"kDrTile = kDrBlk \* kDrPer", src["delivery_report.hpp"])
    return c


def cdiv(a, b):
    return -(-a // b)


def trips(c=None):
    """{loop: (items the loop is given at the size its test uses, items a trip takes)}."""
    c = c or constants()
    fs_blk = c["SBE_FS_PER"] * c["kFsThreads"]
    oj_trip = 4 * c["kScanThreads"]
    return {
        "frag_scan_blocks": (cdiv(N, fs_blk), fs_blk),
        "frag_scan_blocks (B)": (cdiv(N_FRAG_B, fs_blk), fs_blk),
        "tp_frag_scan_blocks": (cdiv(N + 1, fs_blk), fs_blk),  # with a carry the table holds one entry more
        # frag_copy: wave w takes the message groups w, w + waves, ...; N - 1024 messages at the least
        "frag_copy": (cdiv(N - 1024 + 1, c["kFragGroup"]), c["SBE_FC_MAXB"] * 4),
        "mat_scan_blocks": (cdiv(N, c["kMatBlk"]), c["kMatBlk"]),
        "ta_scan_blocks": (cdiv(N + 1, c["kMatBlk"]), c["kMatBlk"]),
        "order_json_scan_blocks": (cdiv(N, c["kBlock"]), oj_trip),
        "order_json_scan_blocks (commit)": (2 * (cdiv(N_COMMIT, c["kBlock"]) + 1), oj_trip),
        "lat_sort tiles": (cdiv(N_LAT, c["kDrBlk"] * c["kDrPer"]), c["kDrSortBlocks"]),
        "lat_report_final": (N_LAT, c["kDrSortBlocks"] * c["kDrBlk"]),
        "dr_list_scan": (INF_SMALL, c["kDrListBlocks"] * c["kDrBlk"]),
        "inf_rehash / inf_reset_values": (INF_BIG, c["kInfRehashBlocks"] * c["kInfBlk"]),
    }


# ------------------------------------------------------------------------------------------
# the pool method
# ------------------------------------------------------------------------------------------
def as_tensor(a, device="cpu"):
    """A numpy array as a tensor of the same width (unsigned types as their signed twins)."""
    a = np.ascontiguousarray(a)
    twin = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}
    if a.dtype in twin:
        a = a.view(twin[a.dtype])
    return torch.from_numpy(a.copy()).to(device)


def draw(n, pool_size, seed):
    """n indices into a pool, drawn with replacement."""
    return np.random.default_rng(seed).integers(0, pool_size, n).astype(np.int64)


def assemble(pool, pool_off, pick, chunk=1 << 18):
    """The ranges pool[pool_off[p]:pool_off[p + 1]] for p in pick, back to back: (stream uint8,
    off int64 [len(pick) + 1]).  Tensors of one device."""
    pool_off = pool_off.to(torch.int64)
    n = int(pick.numel())
    lens = (pool_off[1:] - pool_off[:-1])[pick]
    off = torch.zeros(n + 1, dtype=torch.int64, device=pool.device)
    off[1:] = torch.cumsum(lens, 0)
    out = torch.empty(int(off[n]), dtype=torch.uint8, device=pool.device)
    for lo in range(0, n, chunk):  # the index arrays take eight times the bytes: a piece at a time
        hi = min(n, lo + chunk)
        b, e = int(off[lo]), int(off[hi])
        if e == b:
            continue
        shift = pool_off[pick[lo:hi]] - (off[lo:hi] - b)
        idx = torch.arange(e - b, dtype=torch.int64, device=pool.device) + torch.repeat_interleave(shift, lens[lo:hi])
        out[b:e] = pool[idx]
    return out, off


def rows_offsets(row_len):
    """off [k + 1] of rows of lengths row_len [k] (numpy)."""
    off = np.zeros(len(row_len) + 1, np.int64)
    off[1:] = np.cumsum(np.asarray(row_len, np.int64))
    return off


# ------------------------------------------------------------------------------------------
# reassembly
# ------------------------------------------------------------------------------------------
BEGIN, END, SINGLE, MIDDLE = 0x80, 0x40, 0xC0, 0x00


def oracle_reassemble_arrays(data, frag_off, flags):
    """T.oracle_reassemble without the list of messages: (out = messages then carry, msg_off
    [m + 1], counts [2]) as the device call documents them."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    frag_off = np.ascontiguousarray(frag_off, dtype=np.uint64)
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    n = flags.size
    tot = max(int(frag_off[-1] - frag_off[0]), 1)
    out, acc = np.zeros(tot, np.uint8), np.zeros(tot, np.uint8)
    msg_off, counts = np.zeros(n + 1, np.uint64), np.zeros(2, np.uint64)
    T.oracle().orc_reassemble(T._p(data), T._p(frag_off), T._p(flags), n, T._p(out), T._p(msg_off), T._p(counts),
                              T._p(acc))
    m = int(counts[0])
    return out[: int(msg_off[m]) + int(counts[1])], msg_off[: m + 1], counts


def _frag_data(n, rng):
    lens = rng.integers(0, 9, n)  # 0..8 bytes a fragment
    frag_off = np.zeros(n + 1, np.uint64)
    frag_off[1:] = np.cumsum(lens)
    return rng.integers(0, 256, int(frag_off[-1]), dtype=np.uint8), frag_off


def frag_stream_singles(n=N, seed=0xB16A):
    """Stream (A): almost all whole messages, a few short BEGIN [middle] END groups: more than
    2^20 messages, so the waves of frag_copy stride."""
    rng = np.random.default_rng(seed)
    flags = np.full(n, SINGLE, np.uint8)
    at = np.sort(rng.choice(np.arange(0, n - 3, 4), 256, replace=False))  # disjoint starts
    three = rng.random(at.size) < 0.5
    flags[at] = BEGIN
    flags[at + 1] = np.where(three, MIDDLE, END)
    flags[(at + 2)[three]] = END
    data, frag_off = _frag_data(n, rng)
    return data, frag_off, flags


def group_at(flags, b, e, singles):
    """Writes a BEGIN at b, an END at e, middles between them and whole messages at `singles`."""
    flags[b:e + 1] = MIDDLE
    flags[b], flags[e] = BEGIN, END
    flags[list(singles)] = SINGLE


def is_group(flags, b, e):
    """flags[b..e] is one BEGIN .. END group: no BEGIN or END of a group between them."""
    inner = flags[b + 1:e]
    return bool(flags[b] == BEGIN and flags[e] == END and np.isin(inner, (MIDDLE, SINGLE)).all())


def singles_inside(flags, b, e):
    return int((flags[b + 1:e] == SINGLE).sum())


def frag_streams_structured(blk, seed=0xB16B):
    """Streams (B): {name: (data, frag_off, flags, marks)} of N_FRAG_B fragments with independent
    random flags (so groups, strays, BEGIN over BEGIN and singles inside groups occur throughout)
    and, laid over them at the edge of the second trip of the block scan (scan block `blk`
    fragments; block blk is the first of the second trip):
      edge   a group from block blk - 1 to block blk with singles inside, then in block blk a stray
             END and a BEGIN over a BEGIN
      long   a group from block blk - 4 to block blk + 1 with singles inside
      carry  a BEGIN in block blk - 2 that nothing closes: the open carry
    marks: the indices the tests assert the properties from."""
    rng = np.random.default_rng(seed)
    n, E = N_FRAG_B, blk * blk  # E: the first fragment of block blk
    out = {}
    for name in ("edge", "long", "carry"):
        flags = rng.choice(np.array([SINGLE, BEGIN, END, MIDDLE], np.uint8), n, p=[0.55, 0.12, 0.15, 0.18])
        marks = {}
        if name == "edge":
            b, e = E - 7, E + 5
            group_at(flags, b, e, (E - 3, E, E + 2))
            flags[e + 1] = SINGLE
            flags[e + 2] = END                      # no group is open: a stray END
            flags[e + 3], flags[e + 4], flags[e + 5], flags[e + 6] = BEGIN, MIDDLE, BEGIN, END
            marks = dict(b=b, e=e, stray_end=e + 2, begin1=e + 3, begin2=e + 5)
        elif name == "long":
            b, e = E - 4 * blk + 17, E + blk + 9
            group_at(flags, b, e, ())
            inner = np.arange(b + 1, e)
            flags[inner[rng.random(inner.size) < 0.3]] = SINGLE
            flags[[E - 1, E, E + blk - 1, E + blk]] = SINGLE  # singles at the block edges themselves
            marks = dict(b=b, e=e)
        else:
            b = E - 2 * blk + 100
            flags[b] = BEGIN
            tail = np.arange(b + 1, n)
            flags[tail] = np.where(rng.random(tail.size) < 0.4, SINGLE, MIDDLE)
            marks = dict(b=b)
        data, frag_off = _frag_data(n, rng)
        out[name] = (data, frag_off, flags, marks)
    return out


# ------------------------------------------------------------------------------------------
# term append
# ------------------------------------------------------------------------------------------
TA_MAX_LEN = 40  # max_message_length of the term-append runs: records take 0..40 bytes


def term_append_records(n=N, too_long=(), seed=0xB172):
    """(data uint8, rec_off uint64 [n + 1]): n records of 0..TA_MAX_LEN random non-zero bytes, those
    at the indices `too_long` one byte longer."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, TA_MAX_LEN + 1, n)
    lens[list(too_long)] = TA_MAX_LEN + 1
    rec_off = np.zeros(n + 1, np.uint64)
    rec_off[1:] = np.cumsum(lens)
    return rng.integers(1, 0xA0, int(rec_off[-1]), dtype=np.uint8), rec_off


def term_append_np(block_bytes, start, data, rec_off, mtu=1408, header=TA.HEADER, limit=None,
                   max_message_length=TA_MAX_LEN):
    """termappend_lib.append_offsets in numpy for well-formed records that fit one frame each (or
    are too long), on a block filled with the sentinel: dict(block uint8 array, appended, next,
    payload, stop, rec_tail uint64 array).  test_bigbatch_lib.py holds it to append_offsets and, at
    the sizes of the GPU test, to the host mirror's serial term_append (tests/termappend)."""
    rec_off = np.asarray(rec_off, np.uint64).astype(np.int64)
    n = rec_off.size - 1
    L = np.diff(rec_off)
    assert (L >= 0).all() and rec_off[-1] <= len(data)
    limit = TA.NO_LIMIT if limit is None else limit
    too_long = L > max_message_length
    assert (L[~too_long] <= mtu - TA.HDR).all()
    req = np.where(too_long, 0, (TA.HDR + L + 31) & ~31)
    first_long = int(np.argmax(too_long)) if too_long.any() else n
    before = start + np.cumsum(req) - req  # the tail before record i, as long as no record stopped the call
    k, stop = n, TA.END
    for cond, why in ((before >= min(limit, 1 << 62), TA.LIMIT), (too_long, TA.TOO_LONG), (before + req > block_bytes, TA.TRIPPED)):
        i = int(np.argmax(cond)) if cond.any() else n
        if i < k:  # the earliest record that stops the call; at the same record the loop's order decides
            k, stop = i, why
    assert first_long >= k
    version, session, stream, term, base = header
    block = np.full(block_bytes, TA.SENTINEL, np.uint8)
    at, ln = before[:k], L[:k]
    nxt = int(at[-1] + req[k - 1]) if k else start
    block[start:nxt] = 0
    hdr = np.zeros(k, np.dtype([("length", "<i4"), ("version", "u1"), ("flags", "u1"), ("type", "<u2"), ("offset", "<i4"),
                               ("session", "<i4"), ("stream", "<i4"), ("term", "<i4"), ("reserved", "<i8")]))
    hdr["length"], hdr["version"], hdr["flags"], hdr["type"] = TA.HDR + ln, version, TA.BEGIN | TA.ENDF, 1
    hdr["offset"], hdr["session"], hdr["stream"], hdr["term"] = base + at, session, stream, term
    block[(at[:, None] + np.arange(TA.HDR)).reshape(-1)] = hdr.view(np.uint8)
    total = int(ln.sum())
    if total:
        own = np.repeat(np.arange(k), ln)            # the record of every payload byte
        j = np.arange(total) - np.repeat(rec_off[:k] - rec_off[0], ln)
        block[at[own] + TA.HDR + j] = np.asarray(data)[rec_off[0]: rec_off[k]]
    if stop == TA.TRIPPED:
        if nxt < block_bytes:
            block[nxt: nxt + TA.HDR] = np.frombuffer(TA.frame_header(block_bytes - nxt, TA.BEGIN | TA.ENDF, 0, base + nxt, header), np.uint8)
        nxt = block_bytes
    return dict(block=block, appended=k, next=nxt, payload=int(rec_off[k] - rec_off[0]), stop=stop,
                rec_tail=(at + req[:k]).astype(np.uint64))


def term_append_runs(blk):
    """The three runs of the GPU test as (name, data, rec_off, block bytes, expected stop): every
    record fits; a too-long record in a plan block of the second trip of ta_scan_blocks (blocks
    of `blk` records) and none before it; one in block 3 and one in the second trip."""
    out = []
    for name, long_at, stop in (("fits", (), TA.END), ("late", (blk * blk + 5,), TA.TOO_LONG),
                                ("early and late", (3 * blk + 7, blk * blk + 5), TA.TOO_LONG)):
        data, rec_off = term_append_records(N, long_at)
        frames = int(((TA.HDR + np.diff(rec_off.astype(np.int64)) + 31) & ~31).sum())
        out.append((name, data, rec_off, frames + 96, stop, long_at))
    return out


def write_term_append_case(f, block_bytes, start, data, rec_off, exp, mtu=1408, header=TA.HEADER, limit=None,
                           max_message_length=TA_MAX_LEN):
    """One case of the file tests/termappend/term_append_main.cpp reads (termappend_lib.write_cases'
    layout), with `exp` as the expectation."""
    n = len(rec_off) - 1
    f.write(struct.pack("<11Q", block_bytes, start, TA.NO_LIMIT if limit is None else limit, mtu, max_message_length,
                        len(data), n, exp["appended"], exp["next"], exp["payload"], exp["stop"]))
    version, session, stream, term, base = header
    f.write(struct.pack("<5i", session, stream, term, base, version))
    f.write(np.asarray(data, np.uint8).tobytes())
    f.write(np.asarray(rec_off, np.uint64).tobytes())
    f.write(np.asarray(exp["rec_tail"], np.uint64).tobytes())
    f.write(np.asarray(exp["block"], np.uint8).tobytes())


# ------------------------------------------------------------------------------------------
# term poll
# ------------------------------------------------------------------------------------------
def term_poll_block(n=N, edge=1 << 20, seed=0xB175):
    """A term block of n well-formed data frames, header-only ones (32 bytes) and 64-byte ones mixed,
    and the fragment table a walk of it gives, known by construction: (block, payload, frag_off
    [n + 1], flags [n]).  The frames are term_append_np's (one per record of 0..32 bytes) with the
    flags byte of some rewritten: BEGIN / middle / END groups of 2..4 frames here and there, and
    one from fragment edge - 2 to edge + 1, which lies across `edge` with and without the table
    entry a carry puts in front.  test_bigbatch_lib.py holds the table to termscan_lib.walk."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 33, n)
    lens[rng.random(n) < 0.3] = 0
    frag_off = np.zeros(n + 1, np.uint64)
    frag_off[1:] = np.cumsum(lens)
    payload = rng.integers(1, 256, int(frag_off[-1]), dtype=np.uint8)
    nb = int(((TA.HDR + lens + 31) & ~31).sum())
    made = term_append_np(nb, 0, payload, frag_off, max_message_length=32)
    assert made["stop"] == TA.END and made["appended"] == n and made["next"] == nb
    flags = np.full(n, SINGLE, np.uint8)
    starts = np.arange(0, n - 8, 8)
    starts = starts[(rng.random(starts.size) < 0.02) & (np.abs(starts - edge) > 8)]
    size = rng.integers(2, 5, starts.size)
    flags[starts] = BEGIN
    for k in (1, 2, 3):
        inside = starts[size > k]
        flags[inside + k] = np.where(size[size > k] == k + 1, END, MIDDLE)
    flags[edge - 2: edge + 2] = (BEGIN, MIDDLE, MIDDLE, END)
    block = made["block"]
    block[made["rec_tail"].astype(np.int64) - ((TA.HDR + lens + 31) & ~31) + 5] = flags
    return block, payload, frag_off, flags


def term_poll_expected(block_bytes, payload, frag_off, flags, carry=b""):
    """termpoll_lib.expect for a block whose walk gives the table (payload, frag_off, flags) and
    ends at the block's end, in arrays: dict(counts [6], out = messages then carry, msg_off [m + 1])."""
    c = len(carry)
    data = np.concatenate([np.frombuffer(bytes(carry), np.uint8), payload])
    off, fl = np.asarray(frag_off, np.uint64), np.asarray(flags, np.uint8)
    if c:  # the open accumulator leads the table as a middle fragment
        off, fl = np.concatenate([[np.uint64(0)], off + np.uint64(c)]), np.concatenate([[np.uint8(0)], fl])
    out, msg_off, counts = oracle_reassemble_arrays(data, off, fl)
    return dict(counts=[len(flags), block_bytes, len(payload), TS.END, int(counts[0]), int(counts[1])], out=out,
                msg_off=msg_off)


# ------------------------------------------------------------------------------------------
# inflight tables
# ------------------------------------------------------------------------------------------
KEY_BYTES = 16


def hex_keys(count, seed, lead=b"k"):
    """uint8 [count, 16]: distinct keys, `lead` and fifteen random hex digits."""
    rng = np.random.default_rng(seed)
    v = np.unique(rng.integers(0, 1 << 60, count + count // 8, dtype=np.uint64))
    v = v[rng.permutation(v.size)[:count]]
    assert v.size == count
    nib = (v[:, None] >> (np.arange(14, -1, -1, dtype=np.uint64) * np.uint64(4))) & np.uint64(15)
    keys = np.empty((count, KEY_BYTES), np.uint8)
    keys[:, 0] = lead[0]
    keys[:, 1:] = np.frombuffer(b"0123456789abcdef", np.uint8)[nib.astype(np.int64)]
    return keys


def key_list(keys):
    """The rows of a uint8 [count, 16] array as the bytes objects the models take."""
    raw = keys.tobytes()
    return [raw[i: i + KEY_BYTES] for i in range(0, len(raw), KEY_BYTES)]


def ack_records(keys, ts):
    """(data, rec_off): one full ack (inflight_lib.full_ack) per key, all with timestamp `ts`."""
    import inflight_lib as I
    mark = b"#" * KEY_BYTES
    one = I.full_ack(mark, b"orders", b"c", ts)
    at = one.index(mark)
    recs = np.tile(np.frombuffer(one, np.uint8), (len(keys), 1))
    recs[:, at: at + KEY_BYTES] = keys
    return recs.reshape(-1), np.arange(len(keys) + 1, dtype=np.uint64) * np.uint64(len(one))


def table_entries(words):
    """The live entries of a table whose keys all take 16 bytes, from its slot words (uint64
    [capacity, 8]: word, value, five key words, claim | len << 32): (slots, keys as an S16 array,
    values, answered), in slot order."""
    slots = np.nonzero((words[:, 0] >> np.uint64(62)) == 2)[0]
    w = words[slots]
    assert ((w[:, 7] >> np.uint64(32)) == KEY_BYTES).all() and not w[:, 4:7].any()
    keys = np.ascontiguousarray(w[:, 2:4]).view("S16").reshape(-1)
    return slots, keys, w[:, 1].copy(), (w[:, 0] & np.uint64(1)).astype(bool)


# ------------------------------------------------------------------------------------------
# inputs past 4 GiB
# ------------------------------------------------------------------------------------------
FAR_BYTES = 2 ** 32 + 65536
FAR_RECORDS, FAR_BIG = 129, 64  # the batch of test_gpu_far_input.py; the index of its 20 KB record


def far_records(seed=0xB176):
    """129 mixed records: TopicMessages whose payloads are the hand documents of jsonpaths_lib,
    TopicMessages as the commit tests build them (topics in the headers, sequence numbers), full
    acks, CommitOffsetLite and Lite records, shuffled, and at index FAR_BIG one TopicMessage with a
    20 KB payload.  Returns (records, ids of the acks)."""
    import commitsend_lib as CS
    import inflight_lib as I
    import jsonpaths_lib as J
    rng = np.random.default_rng(seed)
    recs = [T.tm_wire([b"t", b"X", b"m%d" % i, d, b"{}"], i) for i, d in enumerate(d for d in J.hand_docs() if len(d) < 300)][:20]
    assert len(recs) == 20
    heads = [b"{}", b'{"topic":"alpha"}', b'{"topic":"beta"}', b'{"topic":""}', b'{"topic":"gamma"}', b'{"topic":"delta"}']
    for i in range(44):
        mid = bytes([97 + i % 26]) * (1 + i * 7 % 23)
        recs.append(T.tm_wire([b"orders", b"SUBSCRIBE" if i % 11 == 10 else b"X", mid, CS.PSEQ if i % 3 == 0 else CS.P,
                               heads[i % len(heads)]], 1_000_000 + i))
    ack_ids = [b"pub_%d" % (1_760_000_000_000_000_000 + 37 * i) for i in range(30)]
    recs += [I.full_ack(k, b"orders", b"corr%d" % i, 5000 + i) for i, k in enumerate(ack_ids)]
    for tmpl, count in ((301, 17), (201, 17)):
        arena, L, tid, seq = T.lite_records(count, tmpl)
        out, off, st = T.oracle_encode_lite(tmpl, arena, L, tid, seq)
        assert (st == 0).all()
        recs += [out[int(off[i]):int(off[i + 1])].tobytes() for i in range(count)]
    recs = [recs[i] for i in rng.permutation(len(recs))]
    big = T.tm_wire([b"orders", b"X", b"m-big", b'{"_sequence_number": 77, "pad":"' + b"p" * 20_000 + b'"}',
                     b'{"topic":"beta"}'], 9)
    recs.insert(FAR_BIG, big)
    assert len(recs) == FAR_RECORDS and sum(len(r) for r in recs) < 60_000
    return recs, ack_ids


def far_base(rec_off):
    """Where the batch goes in the large tensor: 16-byte aligned, byte 2^32 inside the 20 KB record."""
    return (2 ** 32 - int(rec_off[FAR_BIG]) - 10_000) & ~15


# ------------------------------------------------------------------------------------------
# the latency report
# ------------------------------------------------------------------------------------------
def report_np(lats, pcts=R.REPORT_PERCENTILES):
    """report_lib.report with numpy's stable sort (ties in log order) instead of sorted()."""
    lats = np.asarray(lats, np.int64)
    n = lats.size
    order = np.argsort(lats, kind="stable")
    srt = lats[order]
    idx = [R.percentile_index(p, n) if n else 0 for p in pcts]
    total = int(lats.view(np.uint64).sum(dtype=np.uint64)) if n else 0  # mod 2^64
    return {"count": n,
            "stats": np.array([R.s64(total), srt[0] if n else 0, srt[-1] if n else 0], np.int64),
            "pct_value": np.array([srt[i] if n else 0 for i in idx], np.int64),
            "pct_index": np.array(idx, np.uint64),
            "sorted": srt, "order": order.astype(np.uint32)}


# ------------------------------------------------------------------------------------------
# small decoded records (materialize, term append)
# ------------------------------------------------------------------------------------------
def small_record_pool(count=2048, seed=0xB16C):
    """A pool of tiny records with their oracle descriptors: CommitOffsetLite records (decoded in
    Lite mode) and TopicMessages (parse mode) whose strings take 0..6 bytes, a few with every
    string empty.  Returns (data, rec_off, dec): dec the oracle's arrays, a row per record."""
    rng = np.random.default_rng(seed)
    k = count // 2
    L = rng.integers(0, 7, (k, 2)).astype(np.uint32)
    L[:8] = 0
    arena = rng.integers(32, 127, int(L.sum()), dtype=np.uint8)
    lite, lite_off, st = T.oracle_encode_lite(301, arena, L, rng.integers(1, 4, k).astype(np.uint32),
                                              rng.integers(0, 2 ** 63, k).astype(np.uint64))
    assert (st == 0).all()
    recs = []
    for i in range(count - k):
        f = [bytes(rng.integers(32, 127, int(rng.integers(0, 7)), dtype=np.uint8)) for _ in range(5)]
        recs.append(T.tm_wire(f if i >= 8 else [b""] * 5, int(rng.integers(0, 2 ** 63))))
    tm, tm_off = T.pack_records(recs)
    d_lite, d_tm = T.oracle_decode(lite, lite_off, T.DEC_LITE), T.oracle_decode(tm, tm_off, T.DEC_PARSE)
    assert (d_lite["status"] == T.ST_LITE).all() and (d_tm["status"] == T.ST_TM).all()
    data = np.concatenate([lite, tm])
    off = np.concatenate([lite_off, tm_off[1:] + lite_off[-1]])
    dec = {key: np.concatenate([d_lite[key], d_tm[key]]) for key in d_lite}
    return data, off, dec


class Picked:
    """A batch drawn from a pool: gathers per-record rows and per-record byte ranges by `pick`
    (a tensor on the device the batch is wanted on)."""

    def __init__(self, pick):
        self.pick, self.device = pick, pick.device

    def rows(self, a):
        return as_tensor(a, self.device)[self.pick].contiguous()

    def ranges(self, data, off):
        """(stream, off [n + 1]) of the ranges data[off[p]:off[p + 1]] of the picked records."""
        data = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data
        if len(data) == 0:
            data = np.zeros(1, np.uint8)
        return assemble(as_tensor(data, self.device), as_tensor(np.asarray(off).astype(np.int64), self.device), self.pick)


def materialize_pool(data, rec_off, dec):
    """(arena bytes, offsets [count + 1]) of the pool records' materialized views, record by
    record, from T.oracle_materialize."""
    arena, arena_off = T.oracle_materialize(data, rec_off, dec)
    return arena, arena_off[::5].astype(np.int64)


def materialize_expected(pool_arena, pool_arena_off, view_len, pick):
    """The arena and arena_off [5 n + 1] of the batch `pick` (tensors of one device)."""
    arena, _ = assemble(pool_arena, pool_arena_off, pick)
    off = torch.zeros(5 * pick.numel() + 1, dtype=torch.int64, device=pick.device)
    off[1:] = torch.cumsum(view_len[pick].reshape(-1).to(torch.int64), 0)
    return arena, off
