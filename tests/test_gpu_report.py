"""GPU: the delivery reports (sbe_inflight_list_keys, sbe_latency_append, sbe_latency_report)
against the sequential models of tests/report_lib.py.  Every comparison is exact; rows and entries
a call must not write are prefilled and compared, and tables and logs are compared byte for byte
across the calls that only read them."""
import functools

import numpy as np
import pytest
import torch

import delivery_lib as D
import report_lib as R
from test_delivery_lib import e2e_batches
from test_gpu_contract import dev
from test_gpu_delivery import LOOKUP, NOTE, check, lookup, note
from test_gpu_inflight import acks_for, check_match, match, remember, same

pytestmark = pytest.mark.gpu

TAGS = [1, 0]
FILL = 0xA5
FILL32, FILL64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
NOT_IN, IN, ANS, UNANS = R.LIST_NOT_IN_OTHER, R.LIST_IN_OTHER, R.LIST_ANSWERED, R.LIST_UNANSWERED


def filled(n, dtype):
    return torch.full((n * torch.empty(0, dtype=dtype).element_size(),), FILL, dtype=torch.uint8, device="cuda").view(dtype)


def list_keys(codec, tbl, other=None, flags=0, min_value=0, limit=10, rows=None):
    """One call into prefilled arrays of `rows` rows -> every output array, whole."""
    rows = limit + 2 if rows is None else rows
    out = codec.KeyList(filled(1, torch.int64), filled(rows * 40, torch.uint8).view(rows, 40), filled(rows, torch.int32),
                        filled(rows, torch.int64), filled(rows, torch.uint8))
    tbl.list_keys(other, flags, min_value, limit, out=out)
    return out.numpy()


def check_list(got, exp, limit, what):
    count, rows = exp
    assert int(got["count"][0]) == count, f"{what}: count {int(got['count'][0])}, expected {count}"
    n = min(count, limit)
    assert len(rows) == n
    for j, (k, v, a) in enumerate(rows):
        assert got["key"][j].tobytes() == k.ljust(40, b"\0"), f"{what}: key of row {j}"
        assert (int(got["len"][j]), int(got["value"][j]), int(got["answered"][j])) == (len(k), v, int(a)), f"{what}: row {j}"
    # rows at or past min(count, limit) are not written
    assert (got["key"][n:] == FILL).all() and (got["len"][n:] == FILL32).all(), f"{what}: rows past {n}"
    assert (got["value"][n:] == FILL64).all() and (got["answered"][n:] == FILL).all(), f"{what}: rows past {n}"


def both(codec, tbl, m, other=None, m_other=None, flags=0, min_value=0, limit=10, what=""):
    got = list_keys(codec, tbl, other, flags, min_value, limit)
    check_list(got, R.list_keys(m, m_other, flags, min_value, limit), limit, f"{what} flags {flags} limit {limit}")
    return got


# ------------------------------------------------------------------------------------------
# list_keys: hand cases on capacity-64 tables
# ------------------------------------------------------------------------------------------
EDGE = [b"", b"ab", b"ab\0", b"abc", b"\xff", b"\x7f", b"k" * 40]


@pytest.mark.parametrize("tag_bits", TAGS)
def test_hand_list(codec, tag_bits):
    sent, m_sent = codec.Inflight(64, "cuda", tag_bits), D.Table()
    keys = EDGE + [b"c1", b"c2", b"c3", b"c4"]
    ts = np.arange(10, 10 + len(keys), dtype=np.uint64)
    same(remember(sent, keys, ts), m_sent.remember(keys, ts), "status")
    recv, m_recv = codec.Inflight(128, "cuda", 7), D.Table()  # another capacity, other tag bits
    rk = [b"ab", b"c1", b"zz", b"\xff", b"c3", b"ab\0\0", b"x" * 40]
    check(note(recv, rk), m_recv.note(rk), NOTE, "received")
    # erased entries: c2 leaves the table, c3 leaves `other` and is no member any more
    got, acks = match(codec, sent, acks_for([b"c2"]))
    check_match(got, m_sent.match(acks))
    got, acks = match(codec, recv, acks_for([b"c3"]))
    check_match(got, m_recv.match(acks))
    # answered entries
    check(lookup(sent, [b"c1", b"ab", b"", b"nobody"]), m_sent.lookup([b"c1", b"ab", b"", b"nobody"]), LOOKUP, "lookup")
    before = sent.table.clone(), recv.table.clone()
    missing = R.list_keys(m_sent, m_recv, NOT_IN, limit=64)
    assert missing[0] == 7 and [r[0] for r in missing[1]] == [b"", b"ab\0", b"abc", b"c3", b"c4", b"k" * 40, b"\x7f"]
    for limit in (0, 1, 6, 7, 8, 10, 64):  # count below, equal to and above the limit
        both(codec, sent, m_sent, recv, m_recv, NOT_IN, limit=limit, what="missing")
        both(codec, recv, m_recv, sent, m_sent, NOT_IN, limit=limit, what="extra")
        both(codec, sent, m_sent, recv, m_recv, IN, limit=limit, what="both")
        both(codec, sent, m_sent, limit=limit, what="all")
    for flags in (ANS, UNANS):
        both(codec, sent, m_sent, flags=flags, what="answered")
        both(codec, sent, m_sent, recv, m_recv, flags | NOT_IN, what="answered, missing")
        both(codec, sent, m_sent, recv, m_recv, flags | IN, what="answered, both")
    got = both(codec, sent, m_sent, flags=ANS, min_value=11, what="answered, least value")  # "" has 10
    assert int(got["count"][0]) == 2
    both(codec, sent, m_sent, min_value=2 ** 63, what="no value that large")
    assert torch.equal(sent.table, before[0]) and torch.equal(recv.table, before[1])
    # the same entries after a rehash, wherever they sit now
    sent2 = sent.rehash(256, tag_bits=3)
    both(codec, sent2, m_sent, recv, m_recv, NOT_IN, limit=64, what="after rehash")
    both(codec, sent2, m_sent, flags=ANS, limit=64, what="after rehash, answered")
    both(codec, recv, m_recv, sent2, m_sent, NOT_IN, limit=64, what="after rehash, as other")
    # a table without a valid header holds nothing
    bad = codec.Inflight(64, "cuda", tag_bits)
    bad.table.copy_(sent.table)
    bad.table[28] ^= 0xFF  # the magic
    for limit in (0, 10):
        check_list(list_keys(codec, bad, limit=limit), (0, []), limit, "bad table")
        check_list(list_keys(codec, bad, recv, NOT_IN, limit=limit), (0, []), limit, "bad table")
        check_list(list_keys(codec, recv, bad, NOT_IN, limit=limit), R.list_keys(m_recv, None, NOT_IN, limit=limit), limit, "bad other")
        check_list(list_keys(codec, recv, bad, IN, limit=limit), (0, []), limit, "bad other")


@pytest.mark.parametrize("tag_bits", TAGS)
def test_redelivered_ids_are_the_values_from_two_up(codec, tag_bits):
    msgs, m = codec.Inflight(64, "cuda", tag_bits), D.Table()
    for call in ([b"m1", b"m2", b"m5", b"m2"], [b"m5", b"m5", b"m0"], [b"m5", b"m5"]):
        check(note(msgs, call), m.note(call), NOTE, "note")
    assert R.list_keys(m, min_value=2) == (2, [(b"m2", 2, False), (b"m5", 5, False)])
    for limit in (0, 1, 2, 3, 64):
        both(codec, msgs, m, min_value=2, limit=limit, what="redelivered")
    both(codec, msgs, m, min_value=1, what="every id")
    both(codec, msgs, m, min_value=5, what="five")
    both(codec, msgs, m, min_value=6, what="none")


# ------------------------------------------------------------------------------------------
# list_keys: many workgroups hold candidates; all candidates in one workgroup
# ------------------------------------------------------------------------------------------
CAP = 1 << 16


@functools.lru_cache(maxsize=None)
def random_case(narrow):
    """(keys of `table`, keys of `other`, the keys of `table` alone when they were chosen by slot):
    about 20 000 live keys each."""
    keys = R.random_keys(20000, 11)
    if narrow:  # the keys that pass start their chains in 256 slots: one workgroup's round
        only = R.keys_in_slot_range(300, 13, CAP, 4000, 256)
        return keys + only, keys + [b"other-%d" % i for i in range(300)], frozenset(only)
    pick = np.random.default_rng(12).random(len(keys))
    mine = [k for k, p in zip(keys, pick) if p < 0.8]
    theirs = [k for k, p in zip(keys, pick) if p > 0.2]
    return mine, theirs, None


@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("tag_bits", TAGS)
def test_random_list(codec, tag_bits, narrow):
    mine, theirs, only = random_case(narrow)
    tbl, m = codec.Inflight(CAP, "cuda", tag_bits), D.Table()
    other, mo = codec.Inflight(CAP, "cuda", 9), D.Table()
    same(remember(tbl, mine, np.arange(1, len(mine) + 1, dtype=np.uint64)),
         m.remember(mine, np.arange(1, len(mine) + 1, dtype=np.uint64)), "status")
    same(remember(other, theirs), mo.remember(theirs), "status")
    # answer every third key of a stretch, so that the answered filter splits the candidates
    some = mine[::3][:3000]
    check(lookup(tbl, some), m.lookup(some), LOOKUP, "lookup")
    if narrow:
        words = tbl.table[64:].cpu().numpy().view("<u8").reshape(CAP, 8)
        live = np.nonzero((words[:, 0] >> 62) == 2)[0]
        passing = [s for s in live if words[s, 2:7].tobytes()[: int(words[s, 7] >> 32)] in only]
        assert len(passing) == 300 and 4000 <= min(passing) and max(passing) < 4000 + 256 + 600
    before = tbl.table.clone(), other.table.clone()
    for flags, limit in ((NOT_IN, 64), (NOT_IN, 10), (IN, 64), (NOT_IN | UNANS, 64), (IN | ANS, 33), (0, 64), (ANS, 1), (NOT_IN, 0)):
        first = both(codec, tbl, m, other, mo, flags, limit=limit, what="random") if flags & (IN | NOT_IN) else \
            both(codec, tbl, m, flags=flags, limit=limit, what="random")
        again = list_keys(codec, tbl, other if flags & (IN | NOT_IN) else None, flags, 0, limit)
        for k in first:  # a repeated call writes identical bytes
            assert first[k].tobytes() == again[k].tobytes(), k
    both(codec, other, mo, tbl, m, NOT_IN, limit=64, what="random, the other way")
    both(codec, tbl, m, other, mo, NOT_IN, min_value=len(mine) - 40, limit=64, what="random, least value")
    assert torch.equal(tbl.table, before[0]) and torch.equal(other.table, before[1])


# ------------------------------------------------------------------------------------------
# the latency log
# ------------------------------------------------------------------------------------------
def lookups(codec, code, value):
    return codec.KeyLookups(dev(np.asarray(code, np.uint8)), dev(np.asarray(value, np.uint64)), None)


def check_log(log, m, what):
    assert log.header() == m.header(), what
    lat, tag = log.samples()
    same(lat, np.array([s[0] for s in m.samples], np.int64), f"{what}: lat")
    same(tag, np.array([s[1] for s in m.samples], np.uint64), f"{what}: tag")


def append(codec, log, m, code, value, now_ns, unit_ns, tag_base, what):
    log.append(lookups(codec, code, value), now_ns, unit_ns, tag_base)
    m.append(code, value, now_ns, unit_ns, tag_base)
    check_log(log, m, what)


def test_hand_log(codec):
    log, m = codec.LatencyLog(8, "cuda"), R.Log(8)
    assert log.header() == {"capacity": 8, "count": 0, "dropped": 0}
    F, REP, UNK, NONE, LONG = D.SENT_FIRST, D.SENT_REPEAT, D.SENT_UNKNOWN, D.SENT_NONE, D.SENT_LONG
    # every code interleaved; a send time after `now`; -1 999 999 ns is -1 ms
    code = [NONE, F, REP, F, UNK, F, LONG, F, REP, F]
    value = [7, 1_000_000, 7, 9_000_000, 7, 5_999_999, 7, 4_000_001, 7, 2 ** 64 - 1_000_000]
    append(codec, log, m, code, value, 4_000_000, 1_000_000, 2 ** 64 - 3, "first call")
    assert m.samples == [(3, 2 ** 64 - 2), (-5, 0), (-1, 2), (0, 4), (5, 6)]
    append(codec, log, m, [F, F, REP, F], [10, 20, 30, 2 ** 63], 15, 1, 1000, "fills it exactly")  # unit_ns 1
    assert m.samples[5:] == [(5, 1000), (-5, 1001), (15 - 2 ** 63, 1003)] and m.header()["dropped"] == 0
    append(codec, log, m, [F, UNK, F], [1, 2, 3], 10, 1, 0, "overflows")
    assert m.header() == {"capacity": 8, "count": 8, "dropped": 2}
    append(codec, log, m, [REP, NONE], [1, 2], 10, 1, 0, "nothing to append")
    append(codec, log, m, [], [], 10, 1, 0, "no records")
    append(codec, log, m, [F], [1], 10, 2 ** 62, 0, "still full")
    assert m.header() == {"capacity": 8, "count": 8, "dropped": 3}
    # one slot left: the first sample of a call takes it
    log2, m2 = codec.LatencyLog(3, "cuda"), R.Log(3)
    append(codec, log2, m2, [F, F], [0, 2 ** 63 + 5], 2 ** 63, 2 ** 62, 5, "largest unit")
    assert m2.samples == [(-2, 5), (0, 6)]
    append(codec, log2, m2, [UNK, F, F, F], [0, 8, 9, 10], 0, 3, 2 ** 64 - 1, "one fits")
    assert m2.samples[2] == (-2, 0) and m2.header() == {"capacity": 3, "count": 3, "dropped": 2}
    # a log without a valid header is full and empty
    bad = codec.LatencyLog(8, "cuda")
    bad.log.copy_(log.log)
    bad.log[24] ^= 0xFF  # the magic
    before = bad.log.clone()
    bad.append(lookups(codec, [F, F], [1, 2]), 10, 1, 0)
    assert torch.equal(bad.log, before)
    rep = bad.report((50.0,), want_order=True).numpy()
    assert int(rep["count"][0]) == 0 and list(rep["stats"]) == [0, 0, 0] and list(rep["pct_value"]) == [0]


@pytest.mark.parametrize("n", [255, 256, 257, 2047, 2048, 2049, 70001, 2048 * 256 + 5])
def test_append_sizes(codec, n):
    """Around a wave, a workgroup's 2048 records and the scan's 256 workgroups a round; the later
    calls overflow a log that is part full."""
    rng = np.random.default_rng(n)
    log, m = codec.LatencyLog(n // 3, "cuda"), R.Log(n // 3)
    for call in range(3):
        code = rng.integers(0, 5, n).astype(np.uint8)
        if call == 1:
            code[:] = D.SENT_FIRST  # every record a sample
            code[n // 2:] = D.SENT_REPEAT
        value = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
        append(codec, log, m, code, value, int(rng.integers(0, 2 ** 63)), int(rng.integers(1, 1000)), 2 ** 64 - n, f"call {call}")
    assert m.header()["count"] == n // 3 and m.header()["dropped"] > 0


# ------------------------------------------------------------------------------------------
# the report
# ------------------------------------------------------------------------------------------
def log_of(codec, lats, capacity):
    """A log holding `lats`: unit_ns 1 and now_ns 0, so that lat = -(value) mod 2^64."""
    log = codec.LatencyLog(capacity, "cuda")
    value = np.array([(-int(v)) & R.M64 for v in lats], np.uint64)
    if len(lats):
        log.append(lookups(codec, np.full(len(lats), D.SENT_FIRST, np.uint8), value), 0, 1, 0)
    lat, _ = log.samples()
    same(lat, np.array(lats, np.int64), "the log's samples")
    return log


def check_report(codec, lats, pct=R.REPORT_PERCENTILES, slack=5):
    cap = len(lats) + slack
    log = log_of(codec, lats, cap)
    before = log.log.clone()
    exp = R.report([int(v) for v in lats], pct)
    out = codec.LatencyReport(filled(1, torch.int64), filled(3, torch.int64), filled(max(len(pct), 1) + 1, torch.int64),
                              filled(max(len(pct), 1) + 1, torch.int64), filled(cap, torch.int64), filled(cap, torch.int32))
    log.report(pct, want_order=True, out=out)
    got = out.numpy()
    n = len(lats)
    assert int(got["count"][0]) == n
    same(got["stats"], exp["stats"], "stats")
    same(got["pct_value"][: len(pct)], exp["pct_value"], "pct_value")
    same(got["pct_index"][: len(pct)], exp["pct_index"], "pct_index")
    same(got["sorted"][:n], exp["sorted"], "sorted")
    same(got["order"][:n], exp["order"], "order")
    # entries past count and past n_pct are not written
    assert (got["sorted"][n:].view(np.uint64) == FILL64).all() and (got["order"][n:] == FILL32).all()
    assert got["pct_value"].view(np.uint64)[len(pct)] == FILL64 and got["pct_index"][len(pct)] == FILL64
    plain = log.report(pct).numpy()  # sorted / order null
    assert "sorted" not in plain and int(plain["count"][0]) == n
    same(plain["stats"], exp["stats"], "stats, no order")
    same(plain["pct_value"], exp["pct_value"], "pct_value, no order")
    same(plain["pct_index"], exp["pct_index"], "pct_index, no order")
    assert torch.equal(log.log, before)  # the log is not modified
    return got, exp, log


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2048, 2049])
def test_report_small_counts(codec, n):
    rng = np.random.default_rng(100 + n)
    lats = rng.integers(-50, 50, n)  # negative values and ties
    got, exp, log = check_report(codec, lats, pct=(0.0, 100.0, 99.99) + R.REPORT_PERCENTILES)
    if n == 1:
        assert list(got["pct_value"][:10]) == [int(lats[0])] * 10 and list(got["pct_index"][:10]) == [0] * 10
    if n == 0:
        assert list(got["stats"]) == [0, 0, 0] and list(got["pct_value"][:10]) == [0] * 10 and log.report().average() == 0.0
    else:
        assert log.report().average() == float(int(lats.sum())) / float(n)
    check_report(codec, lats, pct=())


def test_report_thousand_samples_p999_is_the_last(codec):
    lats = np.random.default_rng(3).permutation(1000) * 3 + 7  # distinct
    got, exp, _ = check_report(codec, lats)
    assert list(got["pct_index"][:7]) == [749, 799, 899, 949, 989, 999, 999]
    assert got["pct_value"][5] == got["sorted"][999] == 7 + 3 * 999 and got["sorted"][998] != got["sorted"][999]


def test_report_ties_keep_log_order(codec):
    lats = np.random.default_rng(4).integers(0, 4, 70001)
    got, exp, _ = check_report(codec, lats)
    order = got["order"][:70001].astype(np.int64)
    for v in range(4):  # the positions of equal latencies ascend
        assert (np.diff(order[lats[order] == v]) > 0).all()


def test_report_every_byte_random(codec):
    rng = np.random.default_rng(5)
    lats = rng.integers(R.INT64_MIN, R.INT64_MAX, 70001, dtype=np.int64, endpoint=True)
    lats[[0, 9, 4000, 70000]] = [R.INT64_MAX, R.INT64_MIN, -1, 0]
    lats[5000:5010] = [R.INT64_MIN, R.INT64_MAX, -1, 0, R.INT64_MIN, R.INT64_MAX, -1, 0, 1, -2]
    got, exp, _ = check_report(codec, lats, pct=(0.0, 100.0, 99.99, 50.0) + R.REPORT_PERCENTILES)
    assert int(got["stats"][1]) == R.INT64_MIN and int(got["stats"][2]) == R.INT64_MAX
    assert int(got["stats"][0]) == R.s64(sum(int(v) for v in lats))


def test_report_sum_wraps(codec):
    got, exp, _ = check_report(codec, [R.INT64_MAX, R.INT64_MAX, 5])
    assert list(got["stats"]) == [3, 5, R.INT64_MAX]
    got, exp, _ = check_report(codec, [R.INT64_MIN, R.INT64_MIN, -1])
    assert list(got["stats"]) == [-1, R.INT64_MIN, -1]


def test_report_workspace_for_fewer_samples_than_the_log_holds(codec):
    """The device compares the log's count with what the workspace provides for."""
    lats = np.arange(3000, 0, -1)
    log = log_of(codec, lats, 5000)
    small = torch.empty(codec.lib().sbe_latency_report_workspace_size(2999), dtype=torch.uint8, device="cuda")
    rep = log.report((50.0,), workspace=small).numpy()
    assert int(rep["count"][0]) == 0 and list(rep["stats"]) == [0, 0, 0] and list(rep["pct_value"]) == [0]
    enough = torch.empty(codec.lib().sbe_latency_report_workspace_size(3000), dtype=torch.uint8, device="cuda")
    rep = log.report((50.0,), workspace=enough).numpy()
    assert int(rep["count"][0]) == 3000 and list(rep["stats"]) == [3000 * 3001 // 2, 1, 3000] and list(rep["pct_value"]) == [1500]


# ------------------------------------------------------------------------------------------
# end to end: decode -> extract -> delivery_keys -> note, note, lookup -> append; then the reports
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag_bits", TAGS)
def test_end_to_end_reports(codec, tag_bits):
    sent, batches = e2e_batches()
    msgs, clients, sends = (codec.Inflight(2048, "cuda", tag_bits) for _ in range(3))
    m_msgs, m_clients, m_sends = D.Table(), D.Table(), D.Table()
    log, m_log = codec.LatencyLog(4096, "cuda"), R.Log(4096)
    ts = np.arange(1000, 1000 + len(sent), dtype=np.uint64)
    same(remember(sends, sent, ts), m_sends.remember(sent, ts), "status")
    cb = D.Callback()
    for c, t in zip(sent, ts):
        cb.publish(c, int(t))
    for b, (recs, select) in enumerate(batches):
        data, off, dec, ids, exp = D.parsed(recs, select)
        d, ro, sel = dev(data), dev(off), dev(select)
        ddec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE)
        keys = codec.delivery_keys(ro, ddec, codec.extract_json(d, ro, ddec, codec.ORDER_ID_PATHS, select=sel), select=sel)
        got = keys.numpy()
        buf, cpos, clen = D.patch_escaped(data, got)
        dbuf, dcpos, dclen = dev(buf), dev(cpos), dev(clen)
        msgs.note_keys(dbuf, keys.msg_pos, keys.msg_len, buf_bytes=int(data.size))
        clients.note_keys(dbuf, dcpos, dclen)
        looked = sends.lookup_keys(dbuf, dcpos, dclen)
        now = 10_000 + b
        log.append(looked, now, 1, b << 32)  # right behind the lookup, on its stream
        mk, ck = D.keys_of(buf, exp["msg_pos"], exp["msg_len"]), D.keys_of(buf, cpos, clen)
        m_msgs.note(mk)
        m_clients.note(ck)
        code, value, _ = m_sends.lookup(ck)
        m_log.append(code, value, now, 1, b << 32)
        check_log(log, m_log, f"batch {b}")
        for i in np.nonzero(got["selected"])[0]:
            cb.on_message(*D.strings_of(data, got, i), now)
    short = lambda s: sorted(k for k in s if len(k) <= D.KEY_MAX)  # the host mirror's sets take the longer ids
    # printMessageComparison / printClientOrderAudit: sent and never received, received and never sent
    missing, extra = short(cb.missing()), short(cb.extra())
    assert len(missing) > 10 and len(extra) >= 1
    got = both(codec, sends, m_sends, clients, m_clients, NOT_IN, limit=10, what="missing")
    assert int(got["count"][0]) == len(missing)
    assert [got["key"][j, : got["len"][j]].tobytes() for j in range(10)] == missing[:10]
    got = both(codec, clients, m_clients, sends, m_sends, NOT_IN, limit=64, what="extra")
    assert int(got["count"][0]) == len(extra)
    assert [got["key"][j, : got["len"][j]].tobytes() for j in range(min(64, len(extra)))] == extra[:64]
    # duplicate_delivery_counts: the ids delivered more than once, each with its count
    dup = {k: c for k, c in cb.duplicate_delivery_counts.items() if len(k) <= D.KEY_MAX}
    got = both(codec, msgs, m_msgs, min_value=2, limit=64, what="redelivered")
    assert int(got["count"][0]) == len(dup) > 5
    for j in range(min(64, len(dup))):
        assert dup[got["key"][j, : got["len"][j]].tobytes()] == int(got["value"][j]) - 1
    # printLatencyReport over what the callback's map holds
    lat = {k: v for k, v in cb.client_order_latency.items() if len(k) <= D.KEY_MAX}
    rep = log.report(want_order=True).numpy()
    exp = R.report(m_log.lats())
    n = len(lat)
    assert int(rep["count"][0]) == n > 20 and sorted(lat.values()) == list(rep["sorted"][:n])
    for k in ("stats", "pct_value", "pct_index"):
        same(rep[k], exp[k], k)
    same(rep["sorted"][:n], exp["sorted"], "sorted")
    same(rep["order"][:n], exp["order"], "order")
