"""GPU: the call contract of include/sbecodec.h (its opening comment) for the entry points merged
after tests/test_gpu_contract.py was written: sbe_term_scan, sbe_term_poll, sbe_term_append,
sbe_inflight_list_keys, sbe_latency_log_init / _append / _report, sbe_emit_commit_offsets[_ex],
sbe_inflight_note_keys / _lookup_keys / _reset_values, sbe_delivery_keys, sbe_order_select and
sbe_json_extract_batch.  Four sentences of that comment are pinned, one section each:

  1. "A call writes the output elements its comment names and nothing else: no byte before or after
     an output array, and no byte outside the workspace size it asks for", with every array at the
     alignment the call's own comment promises and no better;
  2. "A workspace needs no particular contents: a call writes every workspace word before it
     reads it";
  3. "Every launch and memset of a call goes to `stream` and to no other stream";
  4. "records a..b of a larger batch are processed by passing rec_off + a with n = b - a ... the
     per-record outputs of that call start at element 0 of the arrays it is given".

Expected values come from the restatements the tests of each call already use (termscan_lib,
termpoll_lib, termappend_lib, report_lib, delivery_lib, commitsend_lib, commitfallback_lib,
select_lib, jsonpaths_lib); every comparison is exact.  Sizes follow the constants of the sources
(bigbatch_lib.constants(), sbe_term_scan_tile(), sbe_term_append_tile())."""
import functools

import numpy as np
import pytest
import torch

import bigbatch_lib as B
import commitfallback_lib as F
import commitsend_lib as CS
import contract_lib as C
import delivery_lib as D
import inflight_lib as I
import jsonpaths_lib as J
import report_lib as R
import select_lib as SL
import termappend_lib as TA
import termpoll_lib as P
import termscan_lib as S
from test_gpu_commit_fallback import Dev
from test_gpu_contract import SUB_N, _need, dec_inputs, dev, on_side_stream, sub_batch, u
from test_gpu_delivery import LOOKUP, NOTE, check, ranges
from test_gpu_inflight import remember, same
from test_gpu_second_trip import LISTS

pytestmark = pytest.mark.gpu

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
SLICES = [(1, 199), (37, 166), (65, 200)]
TERM, SESS = 3, 4


@functools.lru_cache(maxsize=None)
def consts():
    c = B.constants()
    return {"kTaBlk": c["kMatBlk"], "kDrTile": c["kDrBlk"] * c["kDrPer"], "kBlock": c["kBlock"], "kInfBlk": c["kInfBlk"]}


def cuda_bytes(n, fill=0x5A):
    return torch.full((max(int(n), 1),), fill, dtype=U8, device="cuda")


def raw(b):
    return np.frombuffer(bytes(b), np.uint8)


# ------------------------------------------------------------------------------------------
# the term block of the scan and the poll: three tiles and 64 bytes
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def term_block(tile, tiles=3, extra=64, seed=0x5CA7):
    """(block, cases): termscan_lib's random block (singles, BEGIN / middle / END groups, padding
    frames, decoy headers in payloads) over `tiles` tiles and `extra` bytes, so that the last tile is
    partial; cases: (name, start, fragment_limit, frag_capacity)."""
    blk = S.random_block((tiles * tile + extra) // 32, seed)
    assert len(blk) == tiles * tile + extra
    w = S.walk(blk)
    src, fl = w["frag_src"], w["flags"]
    ends = [s + S.align(S.HDR + b - a) for s, a, b in zip(src, w["frag_off"], w["frag_off"][1:])]
    assert w["stop"] == S.END and w["next"] == len(blk)
    assert {0xC0, 0x80, 0x00, 0x40} <= set(fl) and sum(e - s for s, e in zip(src, ends)) < len(blk) - 32 * 32  # padding frames
    for k in range(1, tiles):  # a frame lies across every tile edge
        assert any(s < k * tile < e for s, e in zip(src, ends)), k
    s1 = next(s for s, f in zip(src, fl) if s >= tile + 32 and not f & 0x80)  # no BEGIN: a carry goes into its message
    lim = sum(1 for s in src if s < 2 * tile + tile // 2)
    assert tile < s1 < 2 * tile and 2 * tile <= src[lim - 1] < 3 * tile and lim < w["fragments"]
    cases = [("whole", 0, None, w["fragments"] + 1), ("start-in-tile-1", s1, None, S.walk(blk, s1)["fragments"] + 1),
             ("limit-in-tile-2", 0, lim, lim), ("limit-0", 0, 0, 2), ("start-at-the-end", len(blk), None, 2)]
    return blk, cases


def eff_limit(limit, capacity):
    return capacity if limit is None else min(limit, capacity)


def scan_sizes(codec, nb, start, capacity):
    return dict(out=max(nb - start, 1), frag_off=capacity + 1, flags=max(capacity, 1), frag_src=max(capacity, 1),
                counts=4, workspace=max(int(codec.lib().sbe_term_scan_workspace_size(nb)), 16))


def scan_call(codec, blk_dev, start, limit, capacity, bufs, want_out=True, want_src=True, stream=None):
    codec.term_scan(blk_dev, start, limit, stream=stream, capacity=capacity, out=bufs.get("out"), want_out=want_out,
                    want_src=want_src, workspace=bufs["workspace"], frag_off=bufs["frag_off"], flags=bufs["flags"],
                    frag_src=bufs.get("frag_src"), counts=bufs["counts"])


def scan_expected(blk, start, limit, capacity):
    w = S.walk(blk, start, eff_limit(limit, capacity))
    return dict(counts=[w["fragments"], w["next"], len(w["payload"]), w["stop"]], frag_off=w["frag_off"], flags=w["flags"],
                frag_src=w["frag_src"], out=raw(w["payload"]))


def scan_need(host, poison, exp, keys=("counts", "frag_off", "flags", "frag_src", "out")):
    for k in keys:
        _need(host, poison, k, exp[k])


def test_term_scan_writes_its_outputs_only(codec):
    """sbe_term_scan: counts[0..4), frag_off[0..fragments], flags / frag_src[0..fragments) and the
    payload bytes of out equal the restatement; every element behind them inside the arrays, the
    guard bands and the bytes around a workspace of exactly sbe_term_scan_workspace_size keep the
    poison.  The block is 16-B aligned and not 32, out and the workspace sit at odd addresses,
    frag_off / counts are 8-B and not 16-B, frag_src 4-B and not 8-B aligned (the alignments of
    the call's comment); frag_capacity is the fragment count + 1, or the limit itself."""
    t = codec.term_scan_tile()
    blk, cases = term_block(t)
    blk_dev = C.placed(raw(blk), 16)
    assert blk_dev.data_ptr() % 32 == 16
    nb = len(blk)

    def run_case(start, limit, capacity, want_out, want_src):
        exp = scan_expected(blk, start, limit, capacity)
        sizes = scan_sizes(codec, nb, start, capacity)

        def one(run):
            bufs = {k: run.buf(k, sizes[k], {"frag_off": I64, "counts": I64, "frag_src": I32}.get(k, U8)) for k in sizes
                    if (k != "out" or want_out) and (k != "frag_src" or want_src)}
            assert bufs["workspace"].data_ptr() % 2 == 1 and bufs["frag_off"].data_ptr() % 16 == 8
            scan_call(codec, blk_dev, start, limit, capacity, bufs, want_out, want_src)
            torch.cuda.synchronize()
            run.expect("counts", exp["counts"])
            for k in bufs:
                if k not in ("counts", "workspace"):
                    run.expect_head(k, exp[k])
        C.twice(one)

    for name, start, limit, capacity in cases:
        run_case(start, limit, capacity, True, True)
    run_case(0, None, cases[0][3], False, False)  # frag_src NULL and out NULL
    run_case(cases[1][1], None, cases[1][3], True, False)
    assert np.array_equal(u(blk_dev), raw(blk))


# ------------------------------------------------------------------------------------------
# sbe_term_poll
# ------------------------------------------------------------------------------------------
def poll_sizes(codec, nb, start, capacity, nc):
    return dict(out=max(nc + nb - start, 1), msg_off=capacity + 1, counts=6,
                workspace=max(int(codec.lib().sbe_term_poll_workspace_size(nb, capacity)), 16))


def poll_call(codec, blk_dev, start, limit, capacity, carry_dev, bufs, stream=None):
    codec.term_poll(blk_dev, start, limit, carry=carry_dev, capacity=capacity, out=bufs["out"], msg_off=bufs["msg_off"],
                    workspace=bufs["workspace"], stream=stream, counts=bufs["counts"])


def poll_expected(blk, start, limit, capacity, carry):
    e = P.expect(blk, start, eff_limit(limit, capacity), carry)
    off = np.zeros(len(e["msgs"]) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in e["msgs"]])
    return dict(counts=e["counts"], msg_off=off, out=raw(b"".join(e["msgs"]) + e["carry"]))


def poll_need(host, poison, exp):
    for k in ("counts", "msg_off", "out"):
        _need(host, poison, k, exp[k])


@pytest.mark.parametrize("carry_bytes", [0, 100])
def test_term_poll_writes_its_outputs_only(codec, carry_bytes):
    """sbe_term_poll: the six counts, msg_off[0..m], the messages and the open carry equal
    termpoll_lib; out holds exactly carry_bytes + block_bytes - start bytes ("nothing is written at
    or past out[carry_bytes + block_bytes - start]"), msg_off exactly frag_capacity + 1 entries, the
    workspace exactly sbe_term_poll_workspace_size bytes at an odd address; the carry sits at an odd
    address, the block at 16 mod 32, msg_off / counts at 8 mod 16.  Entries of msg_off past m and
    bytes of out past the carry are unspecified: there, only the guard bands are checked."""
    t = codec.term_scan_tile()
    blk, cases = term_block(t)
    blk_dev = C.placed(raw(blk), 16)
    carry = P.carry_bytes(carry_bytes)
    carry_dev = C.placed(raw(carry), 1) if carry_bytes else None
    nb = len(blk)
    for name, start, limit, capacity in cases:
        exp = poll_expected(blk, start, limit, capacity, carry)
        sizes = poll_sizes(codec, nb, start, capacity, carry_bytes)

        def one(run):
            bufs = {k: run.buf(k, sizes[k], I64 if k in ("msg_off", "counts") else U8) for k in sizes}
            poll_call(codec, blk_dev, start, limit, capacity, carry_dev, bufs)
            torch.cuda.synchronize()
            for k in bufs:
                if k != "workspace":
                    run.expect(k, exp[k])
        C.twice(one)
        if name == "whole":
            assert exp["counts"][4] > 20 and exp["counts"][0] > exp["counts"][4] and len(exp["out"]) > t
    if carry_bytes:
        assert np.array_equal(u(carry_dev), raw(carry))


# ------------------------------------------------------------------------------------------
# sbe_term_append
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def append_records(n, mtu, seed=0, every=3):
    """n records of 0 .. 3 (mtu - 32) bytes: every 128th one of the lengths around the frame
    payload, every `every`-th a few bytes (a 64-byte frame), the others empty (32 bytes)."""
    maxp = mtu - 32
    longs = [3 * maxp, 2 * maxp + 1, maxp + 1, maxp, maxp - 1, 3 * maxp - 1, 2 * maxp, 33]
    recs = []
    for i in range(n):
        ln = longs[(i // 128 + seed) % len(longs)] if i % 128 == 5 else (1 + (i + seed) % 20 if i % every == 0 else 0)
        recs.append(TA.rec(ln, i + seed))
    return recs


def trip_records(recs, mtu, space):
    """recs with the record in front of which 96 bytes or a little more of `space` are left replaced
    by one of 3 (mtu - 32) bytes: it trips, and bytes of the block lie behind the padding header."""
    tail = 0
    for k, r in enumerate(recs):
        if tail + TA.required(len(r), mtu) > space - 96:
            break
        tail += TA.required(len(r), mtu)
    return recs[:k] + [TA.rec(3 * (mtu - 32), 999)] + recs[k + 1:]


def append_call(codec, block, data_dev, off_dev, start, limit, mtu, max_len, bufs, want_tail=True, stream=None):
    codec.term_append(block, data_dev, off_dev, start, limit, mtu, max_len, codec.TermHeader(-9, 77, 0x01020304, 1 << 20, 3),
                      stream=stream, workspace=bufs["workspace"], rec_tail=bufs.get("rec_tail"), want_tail=want_tail,
                      counts=bufs["counts"])


APPEND_HEADER = (3, -9, 77, 0x01020304, 1 << 20)  # version, session, stream, term, term_offset_base


def append_expected(block_fill, nb, start, data, off, mtu, limit, max_len):
    e = TA.append_offsets(bytes([block_fill]) * nb, start, data, off, mtu, APPEND_HEADER, limit, max_len)
    return dict(block=raw(e["block"]), counts=[e["appended"], e["next"], e["payload"], e["stop"]], rec_tail=e["rec_tail"])


@pytest.mark.parametrize("mtu", [64, 1408])
def test_term_append_writes_its_outputs_only(codec, mtu):
    """sbe_term_append: "the call writes every byte of [start, tail of the last appended record) ...
    nothing else in the block and nothing outside it": the whole block of five tiles, at 16 mod 32
    between guard bands, equals termappend_lib's (the bytes in front of `start` and behind the tail
    keep the poison, of a padding frame the 32 header bytes only); counts and rec_tail[0..appended)
    (8 mod 16; or NULL, the tails then live in the workspace) equal it; the workspace has exactly
    sbe_term_append_workspace_size bytes at an odd address.  kTaBlk + 2 records: two plan blocks."""
    t = codec.term_append_tile()
    n = consts()["kTaBlk"] + 2
    maxp = mtu - 32
    recs = append_records(n, mtu, every=2 if mtu == 64 else 3)  # more than three tiles of frames, less than four
    nb, start = 5 * t, t + 96
    assert 3 * t + 64 < TA.exact_block(recs, mtu) <= nb - start
    ws_bytes = int(codec.lib().sbe_term_append_workspace_size(n))
    runs = [("end", start, None, TA.MAX_LEN, TA.END, True), ("end-null-tail", start, None, TA.MAX_LEN, TA.END, False),
            ("tripped", 2 * t - 64, None, TA.MAX_LEN, TA.TRIPPED, True), ("limit", start, 3 * t + 40, TA.MAX_LEN, TA.LIMIT, True),
            ("too-long", start, None, 2 * maxp + 1, TA.TOO_LONG, True)]
    for name, st, limit, max_len, stop, want_tail in runs:
        data, off = TA.pack(trip_records(recs, mtu, nb - st) if stop == TA.TRIPPED else recs, lead=3)
        data_dev, off_dev = C.placed(raw(data), 1), C.placed(np.asarray(off, np.uint64), 8)

        def one(run):
            exp = append_expected(run.poison, nb, st, data, off, mtu, limit, max_len)
            assert exp["counts"][3] == stop and 0 < exp["counts"][0] < n + (stop == TA.END), name
            if stop == TA.TRIPPED:  # the padding header written, nothing behind it
                tail = exp["rec_tail"][-1]
                assert tail < nb - 32 and exp["counts"][1] == nb and (exp["block"][tail + 32:] == run.poison).all()
            block = run.buf("block", nb, U8, align=16)
            bufs = dict(counts=run.buf("counts", 4, I64), workspace=run.buf("workspace", ws_bytes, U8))
            if want_tail:
                bufs["rec_tail"] = run.buf("rec_tail", n, I64)
            assert block.data_ptr() % 32 == 16 and bufs["counts"].data_ptr() % 16 == 8
            append_call(codec, block, data_dev, off_dev, st, limit, mtu, max_len, bufs, want_tail)
            torch.cuda.synchronize()
            run.expect("block", exp["block"])
            run.expect("counts", exp["counts"])
            if want_tail:
                run.expect("rec_tail", exp["rec_tail"])  # i < appended; the rest is unspecified
        C.twice(one)

    def none(run):  # n == 0: one launch that writes counts
        block = run.buf("block", nb, U8, align=16)
        bufs = dict(counts=run.buf("counts", 4, I64), workspace=run.buf("workspace", 16, U8), rec_tail=run.buf("rec_tail", 1, I64))
        append_call(codec, block, data_dev, off_dev[:1], start, None, mtu, TA.MAX_LEN, bufs)
        torch.cuda.synchronize()
        run.expect("counts", [0, start, 0, TA.END])
        for k in ("block", "rec_tail", "workspace"):
            run.expect_poison(k)
    C.twice(none)
    assert np.array_equal(u(data_dev), raw(data))


# ------------------------------------------------------------------------------------------
# sbe_inflight_list_keys
# ------------------------------------------------------------------------------------------
LIST_CAP = 4096


class Tables:
    """Two tables of LIST_CAP slots in guarded 64-B aligned buffers, with their models: `tbl` holds
    remembered keys, a part of them answered; `other` holds noted keys, half of them tbl's."""

    def __init__(self, codec, n_keys=1500):
        self.mem = C.PoisonRun(C.POISONS[0])
        size = codec.Inflight.table_bytes(LIST_CAP)
        self.tbl = codec.Inflight(LIST_CAP, "cuda", 1, table=self.mem.buf("table", size, U8, align=64))
        self.other = codec.Inflight(LIST_CAP, "cuda", 7, table=self.mem.buf("other", size, U8, align=64))
        self.m, self.mo = D.Table(), D.Table()
        keys = R.random_keys(n_keys, 21)
        order = np.random.default_rng(22).permutation(n_keys)
        mine = [keys[i] for i in order[: 2 * n_keys // 3]]
        theirs = [keys[i] for i in order[n_keys // 3:]]
        ts = np.arange(1, len(mine) + 1, dtype=np.uint64)
        same(remember(self.tbl, mine, ts), self.m.remember(mine, ts), "status")
        b, p, l, nb = ranges(theirs)
        check(self.other.note_keys(b, p, l, buf_bytes=nb).numpy(), self.mo.note(theirs), NOTE, "note")
        b, p, l, nb = ranges(mine[::3])
        check(self.tbl.lookup_keys(b, p, l, buf_bytes=nb).numpy(), self.m.lookup(mine[::3]), LOOKUP, "lookup")
        torch.cuda.synchronize()
        self.before = self.tbl.table.clone(), self.other.table.clone()

    def unchanged(self):
        assert torch.equal(self.tbl.table, self.before[0]) and torch.equal(self.other.table, self.before[1])
        self.mem.check_guards()


LIST_TYPES = dict(count=I64, key=U8, len=I32, value=I64, answered=U8)


def list_sizes(codec, limit):
    return dict(count=1, key=40 * limit, len=limit, value=limit, answered=limit,
                workspace=int(codec.lib().sbe_inflight_list_workspace_size(limit)))


def list_call(codec, tabs, flags, limit, bufs, stream=None, min_value=0):
    out = codec.KeyList(bufs["count"], bufs["key"].view(-1 if limit else 0, 40), bufs["len"], bufs["value"], bufs["answered"])
    member = flags & (R.LIST_IN_OTHER | R.LIST_NOT_IN_OTHER)
    tabs.tbl.list_keys(tabs.other if member else None, flags, min_value, limit, out=out, workspace=bufs["workspace"],
                       stream=stream)


def list_expected(tabs, flags, limit, min_value=0):
    member = flags & (R.LIST_IN_OTHER | R.LIST_NOT_IN_OTHER)
    count, rows = R.list_keys(tabs.m, tabs.mo if member else None, flags, min_value, limit)
    return dict(count=[count], key=raw(b"".join(k.ljust(40, b"\0") for k, _, _ in rows)),
                len=np.array([len(k) for k, _, _ in rows], np.uint32), value=np.array([v for _, v, _ in rows], np.uint64),
                answered=np.array([int(a) for _, _, a in rows], np.uint8))


def test_list_keys_writes_its_outputs_only(codec):
    """sbe_inflight_list_keys: count[0] and the rows j < min(count, limit) equal report_lib; "rows at
    or past that are not written"; the row arrays hold exactly `limit` rows (none for limit 0), count
    is 8-B and not 16-B aligned, the workspace has exactly sbe_inflight_list_workspace_size(limit)
    bytes at an odd address; "No call here modifies a table": both tables are byte-identical
    afterwards and the bands around them intact."""
    tabs = Tables(codec)
    seen = set()
    # the filters of test_gpu_second_trip.LISTS, and one that fewer entries pass than the rows hold
    for flags, min_value in [(f, 0) for f, _ in LISTS] + [(R.LIST_ANSWERED, 990)]:
        for limit in (64, 1, 0):
            exp = list_expected(tabs, flags, limit, min_value)
            seen.add(exp["count"][0] > limit)
            sizes = list_sizes(codec, limit)

            def one(run):
                bufs = {k: run.buf(k, sizes[k], LIST_TYPES.get(k, U8)) for k in sizes}
                assert bufs["count"].data_ptr() % 16 == 8
                list_call(codec, tabs, flags, limit, bufs, min_value=min_value)
                torch.cuda.synchronize()
                for k in LIST_TYPES:
                    run.expect_head(k, exp[k])
            C.twice(one)
    assert seen == {True, False}
    tabs.unchanged()


# ------------------------------------------------------------------------------------------
# the latency log
# ------------------------------------------------------------------------------------------
PCT16 = (0.0, 100.0, 99.99, 50.0, 25.0, 10.0, 1.0, 0.01, 33.3) + R.REPORT_PERCENTILES
OTHER_CODES = (D.SENT_NONE, D.SENT_REPEAT, D.SENT_UNKNOWN, D.SENT_LONG)


@functools.lru_cache(maxsize=None)
def lookup_results(samples, seed):
    """(code, value) of a lookup_keys call with `samples` SENT_FIRST records and, behind every
    fourth of them, a record of another code (not recorded)."""
    rng = np.random.default_rng(seed)
    code, value = [], []
    for i in range(samples):
        code.append(D.SENT_FIRST)
        value.append(int(rng.integers(0, 2 ** 40)))
        if i % 4 == 1:
            code.append(OTHER_CODES[(i // 4) % 4])
            value.append(int(rng.integers(0, 2 ** 40)))
    return np.array(code, np.uint8), np.array(value, np.uint64)


LAT_NOW, LAT_UNIT = 2 ** 39, 1000


def lat_appends(codec, log, calls, ws_of, stream=None):
    """calls: (code dev, value dev, tag_base); ws_of(k, n): the workspace of call k."""
    for k, (code, value, tag) in enumerate(calls):
        n = int(code.numel())
        log.append(codec.KeyLookups(code, value, None), LAT_NOW, LAT_UNIT, tag, workspace=ws_of(k, n), stream=stream)


def lat_model(capacity, calls):
    m = R.Log(capacity)
    for code, value, tag in calls:
        m.append(code, value, LAT_NOW, LAT_UNIT, tag)
    return m


def log_expected(m):
    """The bytes of the log's header words and of lat[0..count) / tag[0..count)."""
    h = m.header()
    return (np.array([h["capacity"], h["count"], h["dropped"]], np.uint64), np.array(m.lats(), np.int64),
            np.array([s[1] for s in m.samples], np.uint64))


def check_log_bytes(body, m, poison=None):
    """body: the log as uint8; with `poison`, the sample slots past count still hold it."""
    hdr, lat, tag = log_expected(m)
    cap, cnt = m.capacity, len(m.samples)
    same(body[:24].view(np.uint64), hdr, "log header")
    same(body[64: 64 + 8 * cnt].view(np.int64), lat, "log lat")
    same(body[64 + 8 * cap:][: 8 * cnt].view(np.uint64), tag, "log tag")
    if poison is not None:
        assert (body[64 + 8 * cnt: 64 + 8 * cap] == poison).all() and (body[64 + 8 * (cap + cnt): 64 + 16 * cap] == poison).all()


REPORT_TYPES = dict(count=I64, stats=I64, pct_value=I64, pct_index=I64, sorted=I64, order=I32)


def report_sizes(codec, capacity, n_pct, want_order):
    s = dict(count=1, stats=3, pct_value=max(n_pct, 1), pct_index=max(n_pct, 1),
             workspace=int(codec.lib().sbe_latency_report_workspace_size(capacity)))
    if want_order:
        s.update(sorted=capacity, order=capacity)
    return s


def report_call(codec, log, pct, bufs, stream=None):
    out = codec.LatencyReport(bufs["count"], bufs["stats"], bufs["pct_value"], bufs["pct_index"], bufs.get("sorted"),
                              bufs.get("order"))
    log.report(pct, want_order="sorted" in bufs, out=out, workspace=bufs["workspace"], stream=stream)


def report_expected(m, pct):
    e = R.report(m.lats(), pct)
    e["count"] = [e["count"]]
    return e


def test_latency_log_writes_its_outputs_only(codec):
    """sbe_latency_log_init / _append / _report on a log of 2 kDrTile samples in a guarded 64-B
    aligned buffer: kDrTile + 1 samples in two calls (kDrTile - 3, then 4: the second crosses the
    tile edge) among records of codes that are not recorded, each with a workspace of exactly
    sbe_latency_append_workspace_size(n) bytes (8-B aligned); the log's header and samples equal
    report_lib's, the sample slots past count keep the poison.  The report, with and without sorted /
    order and with 16 and 0 percentiles, into arrays of exactly `capacity` / n_pct entries and a
    workspace of exactly sbe_latency_report_workspace_size(capacity) bytes: everything equals
    report_lib, "the first `count` entries written" (the rest keep the poison), and "the log is not
    modified"."""
    tile = consts()["kDrTile"]
    cap = 2 * tile
    host_calls = [lookup_results(tile - 3, 1) + (2 ** 64 - 5,), lookup_results(4, 2) + (1 << 32,)]
    calls = [(dev(c), C.placed(v, 8), t) for c, v, t in host_calls]
    m = lat_model(cap, host_calls)
    assert len(m.samples) == tile + 1 and any(c.size > (c == D.SENT_FIRST).sum() for c, _, _ in host_calls)

    def one(run):
        log = codec.LatencyLog(cap, "cuda", log=run.buf("log", codec.LatencyLog.log_bytes(cap), U8, align=64))
        lat_appends(codec, log, calls, lambda k, n: run.buf("append_ws%d" % k, int(codec.lib().sbe_latency_append_workspace_size(n)),
                                                           U8, align=8))
        torch.cuda.synchronize()
        check_log_bytes(run["log"].bytes.cpu().numpy(), m, run.poison)
        before = run["log"].raw.clone()
        for v, (pct, want_order) in enumerate(((PCT16, True), (PCT16, False), ((), True), ((), False))):
            sizes = report_sizes(codec, cap, len(pct), want_order)
            bufs = {k: run.buf("%s%d" % (k, v), sizes[k], REPORT_TYPES.get(k, U8)) for k in sizes}
            report_call(codec, log, pct, bufs)
            torch.cuda.synchronize()
            exp = report_expected(m, pct)
            for k in bufs:
                if k != "workspace":
                    run.expect_head("%s%d" % (k, v), exp[k])
        assert torch.equal(run["log"].raw, before)
    C.twice(one)


# ------------------------------------------------------------------------------------------
# 2. workspace contents do not matter
# ------------------------------------------------------------------------------------------
def plain(sizes, types=None):
    """Plain device tensors of sizes[k] elements (one at the least) of types[k] (default uint8)."""
    types = types or {}
    return {k: torch.zeros(max(n, 1), dtype=types.get(k, U8), device="cuda") for k, n in sizes.items()}


def host_of(bufs):
    return {k: u(t) for k, t in bufs.items()}


TERM_TYPES = dict(frag_off=I64, counts=I64, frag_src=I32, msg_off=I64, rec_tail=I64)


def test_term_scan_workspace_contents_do_not_matter(codec):
    """"A workspace needs no particular contents".  sbe_term_scan on one workspace: the four-tile
    block from `start` 0, a two-tile block from a start in its tile 1 on what that left (valid-looking
    rows of tile 0 are then stale), both again after fills of 0xFF and of 0x00.

    Every workspace word a launch reads is written earlier in the same call: term_tile_chain writes
    the w_exit / w_frags / w_bytes rows of every tile from the start's tile on; term_walk_tiles reads
    rows of slots at or behind `start` only (a chain only moves forward), writes visited[0..nv) and,
    on every path, nvisited; term_emit reads nvisited and visited[blockIdx.x] below it."""
    t = codec.term_scan_tile()
    big_blk, cases = term_block(t)
    small_blk = S.random_block(2 * t // 32, 0x5CA8)
    s1 = next(s for s in S.walk(small_blk)["frag_src"] if s >= t + 32)
    big_dev, small_dev = dev(raw(big_blk)), dev(raw(small_blk))

    def runner(blk, blk_dev, start):
        capacity = S.walk(blk, start)["fragments"] + 1
        exp = scan_expected(blk, start, None, capacity)

        def call(ws):
            bufs = plain(scan_sizes(codec, len(blk), start, capacity), TERM_TYPES)
            bufs["workspace"] = ws
            scan_call(codec, blk_dev, start, None, capacity, bufs)
            torch.cuda.synchronize()
            del bufs["workspace"]
            scan_need(host_of(bufs), 0x5A, exp)
        return call

    ws = cuda_bytes(codec.lib().sbe_term_scan_workspace_size(len(big_blk)))
    C.workspace_history(ws, runner(big_blk, big_dev, 0), runner(small_blk, small_dev, s1))


@pytest.mark.parametrize("carry_bytes", [0, 100])
def test_term_poll_workspace_contents_do_not_matter(codec, carry_bytes):
    """"A workspace needs no particular contents".  sbe_term_poll on one workspace, as the scan
    above, with fills of 0xFF, 0x00, 0x80 (BEGIN) and 0xC0 (BEGIN | END): the flag bytes behind the
    delivered count are then plausible fragment flags.

    The walk's part of the workspace: as sbe_term_scan.  The tables: tp_carry_entry writes entry 0,
    term_emit frag_off[0..fragments], flags / frag_src[0..fragments) behind it; tp_frag_reduce writes
    the aggregate of every scan block below n = counts[0] (+ 1), tp_frag_scan_blocks scans those;
    tp_frag_scan_msgs writes msize / mfirst / mlast[0..m]; term_poll_gather reads entries j <= m and
    frag_src of delivered fragments only.  frag_singles_before loads whole aligned 16-byte blocks of
    flags and masks the bytes outside the range it counts, which lies in a scan block in front of
    the caller's own, so below n."""
    t = codec.term_scan_tile()
    big_blk, cases = term_block(t)
    small_blk = S.random_block(2 * t // 32, 0x5CA8)
    s1 = next(s for s in S.walk(small_blk)["frag_src"] if s >= t + 32)
    big_dev, small_dev = dev(raw(big_blk)), dev(raw(small_blk))
    carry = P.carry_bytes(carry_bytes)
    carry_dev = dev(raw(carry)) if carry_bytes else None

    def runner(blk, blk_dev, start, limit):
        capacity = len(blk) // 32 + 1
        exp = poll_expected(blk, start, limit, capacity, carry)

        def call(ws):
            bufs = plain(poll_sizes(codec, len(blk), start, capacity, carry_bytes), TERM_TYPES)
            bufs["workspace"] = ws
            poll_call(codec, blk_dev, start, limit, capacity, carry_dev, bufs)
            torch.cuda.synchronize()
            del bufs["workspace"]
            poll_need(host_of(bufs), 0x5A, exp)
        return call

    ws = cuda_bytes(codec.lib().sbe_term_poll_workspace_size(len(big_blk), len(big_blk) // 32 + 1))
    lim = cases[2][2] // 16 * 16 - 11  # the delivered count is no multiple of 16: flag bytes behind it share its 16-byte block
    C.workspace_history(ws, runner(big_blk, big_dev, 0, None), runner(small_blk, small_dev, s1, None),
                        fills=(0xFF, 0x00, 0x80, 0xC0))
    C.workspace_history(ws, runner(big_blk, big_dev, 0, lim), runner(big_blk, big_dev, cases[1][1], 21),
                        fills=(0xFF, 0x00, 0x80, 0xC0))
    # more than one scan block of fragments, a group across the blocks' edge with singles inside it
    # (frag_singles_before runs), whole and cut inside the group
    edge = P.edge_group_block(1000)
    edge_dev = dev(raw(edge))
    fl = S.walk(edge)["flags"]
    assert fl[1000] == 0x80 and fl.index(0x40) > C.frag_scan_block() + 5
    ws = cuda_bytes(codec.lib().sbe_term_poll_workspace_size(len(edge), len(edge) // 32 + 1))
    C.workspace_history(ws, runner(edge, edge_dev, 0, None), runner(edge, edge_dev, 0, C.frag_scan_block() + 5),
                        fills=(0xFF, 0x00, 0x80, 0xC0))


def test_term_append_workspace_contents_do_not_matter(codec):
    """"A workspace needs no particular contents".  sbe_term_append with rec_tail NULL (the tails
    live in the workspace) on one workspace: a call
    of three plan blocks, one of two on what it left, both again after 0xFF and 0x00.

    ta_sums writes bsum / bmin of every plan block, ta_scan_blocks scans them and writes the plan,
    ta_tails writes tails[0..n) and the counts; ta_write reads the plan and tails below `appended`."""
    t = codec.term_append_tile()
    blk = consts()["kTaBlk"]

    def runner(n, seed, start):
        recs = append_records(n, 64, seed)
        data, off = TA.pack(recs, lead=seed)
        data_dev, off_dev = dev(raw(data)), dev(np.asarray(off, np.uint64))
        nb = start + TA.exact_block(recs, 64) - 96  # the last records trip
        exp = append_expected(0x5A, nb, start, data, off, 64, None, TA.MAX_LEN)
        assert exp["counts"][3] == TA.TRIPPED

        def call(ws):
            bufs = dict(block=cuda_bytes(nb), counts=cuda_bytes(32).view(I64), workspace=ws)
            append_call(codec, bufs["block"], data_dev, off_dev, start, None, 64, TA.MAX_LEN, bufs, want_tail=False)
            torch.cuda.synchronize()
            _need(host_of(bufs), 0x5A, "block", exp["block"])
            _need(host_of(bufs), 0x5A, "counts", exp["counts"])
        return call

    ws = cuda_bytes(codec.lib().sbe_term_append_workspace_size(2 * blk + 9))
    C.workspace_history(ws, runner(2 * blk + 9, 1, 64), runner(blk + 2, 2, t + 32))


def test_list_keys_workspace_contents_do_not_matter(codec):
    """"A workspace needs no particular contents".  sbe_inflight_list_keys on one workspace: limit
    64, then limit 1 with another filter on what it left, both again after 0xFF and 0x00.

    dr_list_scan writes wg_pass and wg_n of every one of its kDrListBlocks workgroups and the first
    wg_n candidates of each; dr_list_merge reads those."""
    tabs = Tables(codec)

    def runner(flags, limit):
        exp = list_expected(tabs, flags, limit)

        def call(ws):
            bufs = plain(list_sizes(codec, limit), LIST_TYPES)
            bufs["workspace"] = ws
            list_call(codec, tabs, flags, limit, bufs)
            torch.cuda.synchronize()
            host = host_of(bufs)
            for k in LIST_TYPES:
                _need(host, 0x5A, k, exp[k])
        return call

    ws = cuda_bytes(codec.lib().sbe_inflight_list_workspace_size(64))
    C.workspace_history(ws, runner(R.LIST_NOT_IN_OTHER, 64), runner(R.LIST_IN_OTHER | R.LIST_ANSWERED, 1))
    tabs.unchanged()


def test_latency_workspaces_contents_do_not_matter(codec):
    """"A workspace needs no particular contents".  sbe_latency_append and sbe_latency_report, each
    on one workspace: a call over three tiles and
    a bit, one over one tile and a bit on what it left, both again after 0xFF and 0x00.

    append: lat_append_count writes the count of every workgroup, lat_append_scan scans them and
    writes the cursor pair, lat_append_place reads both.  report: the buffers are carved for the most
    samples workspace_bytes provides for (so the small log's arrays lie elsewhere than an exactly
    sized workspace would put them); pass p reads key / idx [p & 1] (pass 0 reads the log itself),
    lat_sort_hist writes the 256 rows of every tile below the count, lat_sort_scan scans them,
    lat_sort_scatter writes key / idx [1 - p & 1][0..count); lat_report_final reads [0..count)."""
    tile = consts()["kDrTile"]

    def runner(samples, seed):
        code, value = lookup_results(samples, seed)
        cap = samples + 7
        m = lat_model(cap, [(code, value, 9)])
        calls = [(dev(code), dev(value), 9)]
        exp = report_expected(m, PCT16)

        def append(ws):
            log = codec.LatencyLog(cap, "cuda")
            lat_appends(codec, log, calls, lambda k, n: ws)
            torch.cuda.synchronize()
            check_log_bytes(log.log.cpu().numpy(), m)
            return log

        filled = append(cuda_bytes(codec.lib().sbe_latency_append_workspace_size(int(code.size))))

        def report(ws):
            bufs = plain(report_sizes(codec, cap, len(PCT16), True), REPORT_TYPES)
            bufs["workspace"] = ws
            report_call(codec, filled, PCT16, bufs)
            torch.cuda.synchronize()
            host = host_of(bufs)
            for k in REPORT_TYPES:
                _need(host, 0x5A, k, exp[k])
        return append, report, int(code.size), cap

    big, small = runner(3 * tile + 5, 3), runner(tile + 1, 4)
    C.workspace_history(cuda_bytes(codec.lib().sbe_latency_append_workspace_size(big[2])), big[0], small[0])
    C.workspace_history(cuda_bytes(codec.lib().sbe_latency_report_workspace_size(big[3])), big[1], small[1])


@functools.lru_cache(maxsize=None)
def commit_batch(codec, n, seed):
    return Dev(codec, F.random_records(n, seed), lead=5)


def emit_call(codec, b, fb, bufs, mask=None, stream=None, rows=None):
    """sbe_emit_commit_offsets (fb False) or _ex with the batch's fallback; rows = (a, b): the slice."""
    ro, dec, plan = b.ro, b.gdec, b.gplan
    if rows is not None:
        lo, hi = rows
        ro = ro[lo: hi + 1]
        dec = codec.Decoded(*(getattr(dec, k)[lo:] for k in ("status", "flags", "hdr", "ts", "view_off", "view_len", "seq")))
        plan = codec.CommitPlan(*(getattr(plan, f)[lo:] for f, _ in codec._COMMIT_KEYS[:6]), plan.last, plan.count)
    return codec.emit_commit_offsets(b.d, ro, dec, plan, b.tid, b.itab, mask=mask, session=True, leadership_term_id=TERM,
                                     cluster_session_id=SESS, fallback=b.fb if fb else None, stream=stream, **bufs)


def emit_expected(b, fb, mask=None, rows=None):
    lo, hi = (0, b.n) if rows is None else rows
    off = b.off[lo: hi + 1]
    dec = {k: v[lo:hi] for k, v in b.dec.items()}
    plan = {k: (v if k in ("last", "count") else v[lo:hi]) for k, v in b.plan.items()}
    seq, mask = b.seq[lo:hi], None if mask is None else mask[lo:hi]
    if fb:
        return F.ref_emit(b.data, off, dec, plan, b.topics, b.ids, b.idents, b.default, seq=seq, mask=mask, term=TERM, sess=SESS)
    return CS.ref_emit(b.data, off, dec, plan, b.ids, b.idents, seq=seq, mask=mask, term=TERM, sess=SESS)


def emit_sizes(codec, n, exp):
    return dict(out=int(exp["out_off"][-1]), out_off=n + 1, status=n, emit_idx=n, totals=3,
                workspace=codec.commit_emit_workspace_size(n))


EMIT_TYPES = dict(out_off=I64, emit_idx=I64, totals=I64)


def emit_need(host, poison, exp):
    for k in ("out_off", "status", "emit_idx", "totals", "out"):
        _need(host, poison, k, exp[k])


@pytest.mark.parametrize("fb", [False, True], ids=["plain", "fallback"])
def test_commit_emit_workspace_contents_do_not_matter(codec, fb):
    """"A workspace needs no particular contents".  sbe_emit_commit_offsets and _ex with a fallback
    on one workspace: 600 records (three sizing
    blocks), 257 (two) on what that left, both again after 0xFF and 0x00.

    The measure launch writes sz of every record and both block sums of every sizing block,
    order_json_scan_blocks scans the 2 (nblk + 1) sums in place, the write launch reads them."""
    def runner(n, seed):
        b = commit_batch(codec, n, seed)
        exp = emit_expected(b, fb)
        assert int(exp["totals"][0]) > 20 and (not fb or (exp["status"] == F.EMITTED_JSON).sum() > 5)

        def call(ws):
            bufs = plain(emit_sizes(codec, n, exp), EMIT_TYPES)
            bufs["workspace"] = ws
            emit_call(codec, b, fb, bufs)
            torch.cuda.synchronize()
            emit_need(host_of(bufs), 0x5A, exp)
        return call

    C.workspace_history(cuda_bytes(codec.commit_emit_workspace_size(600)), runner(600, 31), runner(257, 32))


@functools.lru_cache(maxsize=None)
def key_calls(n, seed):
    """(pool, keys): n keys drawn with repeats from a pool of 400, every twelfth record without one."""
    pool = R.random_keys(400, seed)
    rng = np.random.default_rng(seed + 1)
    keys = [None if i % 12 == 7 else pool[int(j)] for i, j in enumerate(rng.integers(0, 400, n))]
    return pool, keys


def test_key_calls_workspace_contents_do_not_matter(codec):
    """"A workspace needs no particular contents".  sbe_inflight_note_keys and
    sbe_inflight_lookup_keys on one workspace each: 3000 records, 1025
    on what they left, both again after 0xFF and 0x00.  inf_note_find / inf_lookup_find write the
    workspace word of every record, the commit launch reads it."""
    def runner(n, seed, lookup):
        pool, keys = key_calls(n, seed)
        b, p, l, nb = ranges(keys)
        ts = np.arange(5, 5 + len(pool) // 2, dtype=np.uint64)

        def call(ws):
            tbl, m = codec.Inflight(LIST_CAP, "cuda", 1), D.Table()
            if lookup:
                same(remember(tbl, pool[::2], ts), m.remember(pool[::2], ts), "status")
                check(tbl.lookup_keys(b, p, l, buf_bytes=nb, workspace=ws).numpy(), m.lookup(keys), LOOKUP, "lookup")
            else:
                check(tbl.note_keys(b, p, l, buf_bytes=nb, workspace=ws).numpy(), m.note(keys), NOTE, "note")
        return call

    for lookup in (False, True):
        C.workspace_history(cuda_bytes(4 * 3000), runner(3000, 41, lookup), runner(1025, 42, lookup))


# ------------------------------------------------------------------------------------------
# 3. the caller's stream
# ------------------------------------------------------------------------------------------
def test_term_scan_runs_on_the_callers_stream(codec):
    """"Every launch and memset of a call goes to `stream`".  sbe_term_scan: the three launches of a
    walk, and the one launch of a limit-0 call: made on a side stream while the current stream is
    busy, every output is complete when that stream alone has been synchronised."""
    t = codec.term_scan_tile()
    blk, cases = term_block(t)
    blk_dev = dev(raw(blk))
    for start, limit, capacity in ((0, None, cases[0][3]), (0, 0, 2)):
        exp = scan_expected(blk, start, limit, capacity)
        bufs = plain(scan_sizes(codec, len(blk), start, capacity), TERM_TYPES)
        on_side_stream(bufs, lambda s: scan_call(codec, blk_dev, start, limit, capacity, bufs, stream=s),
                       lambda host, poison: scan_need(host, poison, exp))


def test_term_poll_runs_on_the_callers_stream(codec):
    """"Every launch is enqueued on `stream`".  sbe_term_poll with a carry: the eight launches of a
    poll, and the two of a limit-0 call (counts, the carry's copy)."""
    t = codec.term_scan_tile()
    blk, cases = term_block(t)
    blk_dev = dev(raw(blk))
    carry = P.carry_bytes(100)
    carry_dev = dev(raw(carry))
    for start, limit, capacity in ((0, None, cases[0][3]), (0, 0, 2)):
        exp = poll_expected(blk, start, limit, capacity, carry)
        bufs = plain(poll_sizes(codec, len(blk), start, capacity, len(carry)), TERM_TYPES)
        on_side_stream(bufs, lambda s: poll_call(codec, blk_dev, start, limit, capacity, carry_dev, bufs, stream=s),
                       lambda host, poison: poll_need(host, poison, exp))


def test_term_append_runs_on_the_callers_stream(codec):
    """"n == 0: one launch that writes counts (END); otherwise four launches on `stream`".
    sbe_term_append: both; the block starts as poison, so a byte a late launch had not written yet
    differs."""
    t = codec.term_append_tile()
    n = consts()["kTaBlk"] + 2
    recs = append_records(n, 1408)
    data, off = TA.pack(recs, lead=3)
    data_dev, off_dev = dev(raw(data)), dev(np.asarray(off, np.uint64))
    nb, start = 5 * t, t + 96
    for count in (n, 0):
        bufs = plain(dict(block=nb, rec_tail=max(count, 1), counts=4,
                          workspace=max(int(codec.lib().sbe_term_append_workspace_size(count)), 16)), TERM_TYPES)

        def verify(host, poison):
            exp = append_expected(poison, nb, start, data, off[: count + 1], 1408, None, TA.MAX_LEN)
            assert exp["counts"][0] == count
            for k in ("block", "counts", "rec_tail"):
                _need(host, poison, k, exp[k])

        on_side_stream(bufs, lambda s: append_call(codec, bufs["block"], data_dev, off_dev[: count + 1], start, None, 1408,
                                                   TA.MAX_LEN, bufs, stream=s), verify)


def test_list_keys_runs_on_the_callers_stream(codec):
    """sbe_inflight_list_keys: "Two launches on `stream`"."""
    tabs = Tables(codec)
    flags, limit = R.LIST_NOT_IN_OTHER, 64
    exp = list_expected(tabs, flags, limit)
    assert exp["count"][0] > limit
    bufs = plain(list_sizes(codec, limit), LIST_TYPES)

    def verify(host, poison):
        for k in LIST_TYPES:
            _need(host, poison, k, exp[k])

    on_side_stream(bufs, lambda s: list_call(codec, tabs, flags, limit, bufs, stream=s), verify)
    tabs.unchanged()


def test_latency_log_runs_on_the_callers_stream(codec):
    """sbe_latency_log_init (one launch), sbe_latency_append ("Three launches on `stream`") and
    sbe_latency_report ("A memset of stats and 25 launches on `stream`") in one call sequence: the
    log itself starts as poison, so an init or append left behind shows in the log and the report."""
    tile = consts()["kDrTile"]
    cap = 2 * tile
    code, value = lookup_results(tile + 1, 5)
    calls = [(dev(code), dev(value), 77)]
    m = lat_model(cap, [(code, value, 77)])
    exp = report_expected(m, PCT16)
    bufs = plain(report_sizes(codec, cap, len(PCT16), True), REPORT_TYPES)
    bufs["append_ws"] = cuda_bytes(codec.lib().sbe_latency_append_workspace_size(int(code.size)))
    log = codec.LatencyLog(cap, "cuda")
    bufs["log"] = log.log

    def call(s):
        log.clear(stream=s)
        lat_appends(codec, log, calls, lambda k, n: bufs["append_ws"], stream=s)
        report_call(codec, log, PCT16, bufs, stream=s)

    def verify(host, poison):
        check_log_bytes(host["log"], m, poison)
        for k in REPORT_TYPES:
            _need(host, poison, k, exp[k])

    on_side_stream(bufs, call, verify)


@pytest.mark.parametrize("fb", [False, True], ids=["plain", "fallback"])
def test_commit_emit_runs_on_the_callers_stream(codec, fb):
    """"Every launch and memset of a call goes to `stream`".  sbe_emit_commit_offsets and _ex with a
    fallback over 600 records (three sizing blocks): the measure launch, the scan of the block sums
    and the write launch."""
    n = 600
    assert n > 2 * consts()["kBlock"]
    b = commit_batch(codec, n, 31)
    exp = emit_expected(b, fb)
    bufs = plain(emit_sizes(codec, n, exp), EMIT_TYPES)
    on_side_stream(bufs, lambda s: emit_call(codec, b, fb, bufs, stream=s), lambda host, poison: emit_need(host, poison, exp))


def test_key_calls_run_on_the_callers_stream(codec):
    """"Every launch and memset of a call goes to `stream`".  sbe_inflight_note_keys and
    sbe_inflight_lookup_keys (a memset of totals and two launches each) and
    sbe_inflight_reset_values (one launch), on a table the call sequence clears and fills itself: a
    second note_keys behind the reset reports every key's count from one delivery, which it does
    only if the reset ran before it."""
    n = 2 * consts()["kInfBlk"] + 5
    pool, keys = key_calls(n, 43)
    b, p, l, nb = ranges(keys)
    arena, koff, klen = (dev(a) for a in I.pack_keys(pool[::2]))
    ts = dev(np.arange(5, 5 + len(pool) // 2, dtype=np.uint64))
    tbl, m = codec.Inflight(LIST_CAP, "cuda", 1), D.Table()
    m.remember(pool[::2], np.arange(5, 5 + len(pool) // 2, dtype=np.uint64))
    exp = dict(zip(("note_code", "note_count", "note_totals"), m.note(keys)))
    exp.update(zip(("look_code", "look_value", "look_totals"), m.lookup(keys)))
    m.reset_values()
    exp.update(zip(("again_code", "again_count", "again_totals"), m.note(keys)))
    assert (exp["note_count"] != exp["again_count"]).sum() > 100
    bufs = plain(dict(rem_status=len(pool) // 2, rem_ws=4 * len(pool), ws=4 * n, note_code=n, note_count=n, note_totals=2,
                      look_code=n, look_value=n, look_totals=3, again_code=n, again_count=n, again_totals=2),
                 dict(note_count=I32, note_totals=I64, look_value=I64, look_totals=I64, again_count=I32, again_totals=I64))

    def call(s):
        tbl.clear(stream=s)
        tbl.remember(arena, koff, klen, ts, stream=s, status=bufs["rem_status"], workspace=bufs["rem_ws"])
        tbl.note_keys(b, p, l, buf_bytes=nb, code=bufs["note_code"], count=bufs["note_count"], totals=bufs["note_totals"],
                      workspace=bufs["ws"], stream=s)
        tbl.lookup_keys(b, p, l, buf_bytes=nb, code=bufs["look_code"], value=bufs["look_value"], totals=bufs["look_totals"],
                        workspace=bufs["ws"], stream=s)
        tbl.reset_values(stream=s)
        tbl.note_keys(b, p, l, buf_bytes=nb, code=bufs["again_code"], count=bufs["again_count"], totals=bufs["again_totals"],
                      workspace=bufs["ws"], stream=s)

    def verify(host, poison):
        for k in exp:
            _need(host, poison, k, exp[k])

    on_side_stream(bufs, call, verify)


@functools.lru_cache(maxsize=None)
def delivery_case(n=SUB_N, seed=61):
    recs, select = D.delivery_batch(seed, n, D.client_ids(40, 3))
    return (select,) + D.parsed(recs, select)


DK_TYPES = {"pos": I64, "len": I32}


def delivery_inputs(codec, off, dec, select, ids):
    return (dev(off), dec_inputs(codec, dec), dev(select),
            codec.JsonFields(dev(ids["doc"]), dev(ids["root_kind"]), dev(ids["kind"]), dev(ids["off"]), dev(ids["len"])))


def test_delivery_keys_runs_on_the_callers_stream(codec):
    """"Every launch and memset of a call goes to `stream`": sbe_delivery_keys' memset of totals and
    its launch."""
    select, data, off, dec, ids, exp = delivery_case(600, 62)
    n = off.size - 1
    ro, ddec, sel, dids = delivery_inputs(codec, off, dec, select, ids)
    bufs = plain(dict({k: n for k in D.KEY_FIELDS}, totals=2), dict({k: DK_TYPES.get(k[-3:], U8) for k in D.KEY_FIELDS}, totals=I64))
    out = codec.DeliveryKeys(*(bufs[k] for k in D.KEY_FIELDS), bufs["totals"])

    def verify(host, poison):
        for k in D.KEY_FIELDS + ("totals",):
            _need(host, poison, k, exp[k])

    on_side_stream(bufs, lambda s: codec.delivery_keys(ro, ddec, dids, select=sel, out=out, stream=s), verify)


# ------------------------------------------------------------------------------------------
# 4. slices of a larger batch
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [False, True], ids=["plain", "fallback"])
@pytest.mark.parametrize("a,b", SLICES)
def test_commit_emit_on_a_slice_of_a_batch(codec, a, b, fb):
    """sbe_emit_commit_offsets[_ex] with rec_off + a, status + a, view_off + 5 a, cm + a, ... of a
    batch classified whole (flags 0 and a mask; SBE_CE_LAST_ONLY is left out, plan->last holds
    indices of the classify call): "the per-record outputs of that call start at element 0 of the
    arrays it is given", so the result equals the restatement run on the slice as a batch of its
    own: out_off[0] == 0, emit_idx relative to the slice, and the uuid of JSON record i ends in
    uuid_ns + (i - a).  The arrays are sized for the whole batch: the elements behind the slice's
    keep the poison, and so do the elements [0, a) and [b, n) of a second set that receives the
    slice in place (out_off + a, status + a, emit_idx + a)."""
    bt = commit_batch(codec, SUB_N, 33)
    N, n = bt.n, b - a
    assert N == SUB_N and int(bt.off[a]) > 0
    mask = (np.arange(N) % 5 != 2).astype(np.uint8)
    mask_dev = dev(mask)
    exp = emit_expected(bt, fb, mask, (a, b))
    m = int(exp["totals"][0])
    assert m > 5 and exp["out_off"][0] == 0 and (exp["status"][mask[a:b] == 0] == F.NONE).all()
    cap = int(exp["out_off"][-1])

    def one(run):
        bufs = dict(out=run.buf("out", cap, U8), out_off=run.buf("out_off", N + 1, I64), status=run.buf("status", N, U8),
                    emit_idx=run.buf("emit_idx", N, I64), totals=run.buf("totals", 3, I64))
        emit_call(codec, bt, fb, bufs, mask=mask_dev[a:], rows=(a, b))
        place = dict(out=run.buf("out2", cap, U8), out_off=run.buf("out_off2", N + 1, I64)[a:], status=run.buf("status2", N, U8)[a:],
                     emit_idx=run.buf("emit_idx2", N, I64)[a:], totals=run.buf("totals2", 3, I64))
        emit_call(codec, bt, fb, place, mask=mask_dev[a:], rows=(a, b))
        torch.cuda.synchronize()
        for k in ("out_off", "status", "out"):
            run.expect_head(k, exp[k])
            run.expect_rows(k + "2", exp[k], 0 if k == "out" else a)
        run.expect_head("emit_idx", exp["emit_idx"])
        run.expect("emit_idx2", exp["emit_idx"], lo=a)
        run.expect_poison("emit_idx2", 0, 8 * a)
        run.expect_poison("emit_idx2", 8 * b)
        run.expect("totals", exp["totals"])
        run.expect("totals2", exp["totals"])
    C.twice(one)
    if fb:  # the uuid counts from the slice's own element 0
        js = np.nonzero(exp["status"] == F.EMITTED_JSON)[0]
        assert js.size > 3 and js[-1] > 0
        for j in (int(js[0]), int(js[-1])):
            assert b"_%d" % (F.UUID0 + j) in F.frame(exp, j) and b"_%d" % (F.UUID0 + j + a) not in F.frame(exp, j)


@pytest.mark.parametrize("a,b", SLICES)
def test_json_extract_and_delivery_keys_on_a_slice_of_a_batch(codec, a, b):
    """sbe_json_extract_batch (with descriptors and a select mask) and sbe_delivery_keys with
    rec_off + a, select + a, view_off + 5 a, kind + 9 a, ...: rows a..b of arrays sized for the whole
    batch equal rows a..b of the whole-batch result (ranges relative to the record start; key
    positions index the batch buffer), the rows outside keep the poison, and the totals are the
    slice's."""
    select, data, off, dec, ids, exp = delivery_case()
    N, n, P9 = SUB_N, b - a, len(J.ORDER_ID_PATHS)
    assert off.size == N + 1 and (select == 0).any() and exp["selected"][a:b].sum() > n // 4
    exp_slice = D.expected_keys(off[a: b + 1], {k: v[a:b] for k, v in dec.items()}, select[a:b], {k: v[a:b] for k, v in ids.items()})
    for k in D.KEY_FIELDS:
        assert np.array_equal(exp_slice[k], exp[k][a:b]), k
    d, ro, sel, ddec = dev(data), C.placed(off, 16), dev(select), dec_inputs(codec, dec)
    rows = codec.Decoded(*(getattr(ddec, k)[a:] for k in ("status", "flags", "hdr", "ts", "view_off", "view_len")))
    jx = dict(doc=(1, U8), root_kind=(1, U8), kind=(P9, U8), off=(P9, I32), len=(P9, I32))

    def one(run):
        full = {k: run.buf(k, per * N, t).view(N, per) if per > 1 else run.buf(k, N, t) for k, (per, t) in jx.items()}
        got = codec.extract_json(d, ro[a: b + 1], rows, codec.ORDER_ID_PATHS, select=sel[a:],
                                 out=codec.JsonFields(*(full[k][a:] for k in jx)))
        keys = {k: run.buf(k, N, DK_TYPES.get(k[-3:], U8)) for k in D.KEY_FIELDS}
        totals = run.buf("totals", 2, I64)
        codec.delivery_keys(ro[a: b + 1], rows, got, select=sel[a:],
                            out=codec.DeliveryKeys(*(keys[k][a:] for k in D.KEY_FIELDS), totals))
        torch.cuda.synchronize()
        for k, (per, _) in jx.items():
            run.expect_rows(k, ids[k][a:b], a, per)
        for k in D.KEY_FIELDS:
            run.expect_rows(k, exp[k][a:b], a)
        run.expect("totals", exp_slice["totals"])
    C.twice(one)


@pytest.mark.parametrize("a,b", SLICES)
def test_order_select_on_a_slice_of_a_batch(codec, a, b):
    """sbe_order_select with rec_off + a, status + a, hdr + 4 a, view_off + 5 a: rows a..b equal rows
    a..b of the whole-batch model, the rows outside keep the poison, the totals are the slice's."""
    data, off, dec, _ = sub_batch()
    N = SUB_N
    whole = SL.model(data, off, dec)
    exp = SL.model(data, off[a: b + 1], {k: v[a:b] for k, v in dec.items()})
    for k in ("pred", "select", "topic_class"):
        assert np.array_equal(exp[k], whole[k][a:b]), k
    assert exp["totals"][1] > 0 and exp["totals"][1] < whole["totals"][1]
    d, ro, ddec = dev(data), C.placed(off, 16), dec_inputs(codec, dec)
    rows = codec.Decoded(*(getattr(ddec, k)[a:] for k in ("status", "flags", "hdr", "ts", "view_off", "view_len")))

    def one(run):
        full = {k: run.buf(k, N, U8) for k in ("pred", "select", "topic_class")}
        out = codec.MessageKinds(*(full[k][a:] for k in full), run.buf("totals", 2, I64))
        codec.order_select(d, ro[a: b + 1], rows, out=out)
        torch.cuda.synchronize()
        for k in full:
            run.expect_rows(k, exp[k], a)
        run.expect("totals", exp["totals"])
    C.twice(one)


@pytest.mark.parametrize("a,b", SLICES)
def test_term_append_on_a_slice_of_a_batch(codec, a, b):
    """sbe_term_append with rec_off + a, n = b - a and in_bytes of the whole input (rec_off indexes
    `in`): the block equals the restatement over the slice; rec_tail + a of an array sized for the
    whole batch is filled in place, the elements outside the slice keep the poison."""
    mtu = 96
    recs = append_records(SUB_N, mtu, 7)
    data, off = TA.pack(recs, lead=5)
    data_dev, off_dev = dev(raw(data)), C.placed(np.asarray(off, np.uint64), 16)
    n, start = b - a, 64
    nb = start + TA.exact_block(recs[a:b], mtu) + 32
    assert off[a] > 0
    ws_bytes = int(codec.lib().sbe_term_append_workspace_size(n))

    def one(run):
        exp = append_expected(run.poison, nb, start, data, off[a: b + 1], mtu, None, TA.MAX_LEN)
        assert exp["counts"] == [n, nb - 32, off[b] - off[a], TA.END]
        block = run.buf("block", nb, U8, align=16)
        tails = run.buf("rec_tail", SUB_N, I64)
        bufs = dict(rec_tail=tails[a:b], counts=run.buf("counts", 4, I64), workspace=run.buf("workspace", ws_bytes, U8))
        append_call(codec, block, data_dev, off_dev[a: b + 1], start, None, mtu, TA.MAX_LEN, bufs)
        torch.cuda.synchronize()
        run.expect("block", exp["block"])
        run.expect("counts", exp["counts"])
        run.expect_rows("rec_tail", exp["rec_tail"], a)
    C.twice(one)
