"""CPU: the sequential models of tests/report_lib.py against transcriptions of the example's three
reports (examples/pubsub_reconnect_test.cpp:130-204, :206-274, :276-353), on hand cases."""
import math

import numpy as np

import delivery_lib as D
import report_lib as R


# ------------------------------------------------------------------------------------------
# the example's code, line for line
# ------------------------------------------------------------------------------------------
def example_comparison(sent, received):
    """:147-163: two std::set<std::string>; iterating one yields it in std::string order."""
    missing, extra = set(), set()
    for cid in sent:
        if cid not in received:
            missing.add(cid)
    for cid in received:
        if cid not in sent:
            extra.add(cid)
    return sorted(missing), sorted(extra)


def example_latency_report(latency):
    """:288-348 over the map client_order_id -> latency."""
    rows = [(lat, cid) for cid, lat in latency.items()]
    latencies = [lat for _, lat in latency.items()]
    rows.sort(key=lambda r: -r[0])  # :304, by latency descending
    out = {"total": len(rows), "rows": [r[0] for r in rows]}
    if latencies:
        latencies.sort()

        def percentile(pct):
            rank = (pct / 100.0) * float(len(latencies))
            idx = 0 if rank <= 0.0 else int(math.ceil(rank)) - 1
            if idx >= len(latencies):
                idx = len(latencies) - 1
            return latencies[idx]

        total = 0
        for v in latencies:
            total += v
        out["average"] = float(total) / float(len(latencies))
        out["pct"] = [percentile(p) for p in R.REPORT_PERCENTILES]
    return out


def table(keys, values=None, answered=()):
    t = D.Table()
    for i, k in enumerate(keys):
        t.inflight[k] = 1 if values is None else values[i]
    t.used = len(keys)
    t.answered = set(answered)
    return t


# ------------------------------------------------------------------------------------------
# list_keys
# ------------------------------------------------------------------------------------------
EDGE = [b"", b"ab", b"ab\0", b"abc", b"\x7f", b"\xff", b"k" * 40]


def test_key_order_is_std_string_order():
    # bytes as unsigned, a proper prefix first: what std::string::compare gives
    n, rows = R.list_keys(table(list(reversed(EDGE))), limit=64)
    assert n == 7 and [r[0] for r in rows] == [b"", b"ab", b"ab\0", b"abc", b"k" * 40, b"\x7f", b"\xff"]


def test_differences_are_the_examples_sets():
    sent = [b"c%03d" % i for i in range(40)] + EDGE
    received = [b"c%03d" % i for i in range(0, 40, 3)] + [b"x1", b"x0", b"ab", b"\xff\x00"]
    missing, extra = example_comparison(set(sent), set(received))
    ts, tr = table(sent), table(received)
    n, rows = R.list_keys(ts, tr, R.LIST_NOT_IN_OTHER, limit=10)
    assert n == len(missing) == 32 and [r[0] for r in rows] == missing[:10]  # the ten the example prints
    n, rows = R.list_keys(tr, ts, R.LIST_NOT_IN_OTHER, limit=10)
    assert n == len(extra) == 3 and [r[0] for r in rows] == extra == [b"x0", b"x1", b"\xff\x00"]
    n, rows = R.list_keys(ts, tr, R.LIST_IN_OTHER, limit=64)
    assert n == 15 and [r[0] for r in rows] == sorted(set(sent) & set(received))
    assert R.list_keys(ts, tr, R.LIST_NOT_IN_OTHER, limit=0) == (32, [])
    # a table without a valid header: nothing as `table`, no member as `other`
    assert R.list_keys(None, tr, R.LIST_NOT_IN_OTHER) == (0, [])
    assert R.list_keys(tr, None, R.LIST_NOT_IN_OTHER, limit=64)[0] == len(received)
    assert R.list_keys(tr, None, R.LIST_IN_OTHER) == (0, [])


def test_answered_and_least_value_filters():
    t = table([b"m1", b"m2", b"m3", b"m4"], [1, 2, 5, 2], answered=[b"m2", b"m3"])
    # duplicate_delivery_counts (:83-90): the ids delivered more than once, each with its count
    assert R.list_keys(t, min_value=2) == (3, [(b"m2", 2, True), (b"m3", 5, True), (b"m4", 2, False)])
    assert R.list_keys(t, flags=R.LIST_ANSWERED) == (2, [(b"m2", 2, True), (b"m3", 5, True)])
    assert R.list_keys(t, flags=R.LIST_UNANSWERED, min_value=2) == (1, [(b"m4", 2, False)])
    assert R.list_keys(t, min_value=6) == (0, [])
    assert R.list_keys(t, min_value=0, limit=1) == (4, [(b"m1", 1, False)])


# ------------------------------------------------------------------------------------------
# the log
# ------------------------------------------------------------------------------------------
def test_append_truncates_toward_zero_and_drops_what_does_not_fit():
    log = R.Log(4)
    code = [D.SENT_FIRST, D.SENT_REPEAT, D.SENT_FIRST, D.SENT_UNKNOWN, D.SENT_FIRST, D.SENT_NONE, D.SENT_LONG]
    value = [1_000_000, 7, 5_999_999, 7, 3_000_000, 7, 7]
    log.append(code, value, now_ns=4_000_000, unit_ns=1_000_000, tag_base=2 ** 64 - 1)
    # 3 ms; -1 999 999 ns is -1 ms, not -2 (duration_cast truncates); 1 ms
    assert log.samples == [(3, 2 ** 64 - 1), (-1, 1), (1, 3)] and log.header() == {"capacity": 4, "count": 3, "dropped": 0}
    log.append([D.SENT_FIRST] * 3, [10, 20, 2 ** 64 - 5], now_ns=15, unit_ns=1, tag_base=100)
    assert log.samples[3] == (5, 100) and log.header() == {"capacity": 4, "count": 4, "dropped": 2}
    assert R.cdiv(-1_999_999, 1_000_000) == -1 and R.cdiv(1_999_999, 1_000_000) == 1 and R.cdiv(-2_000_000, 1_000_000) == -2
    assert R.s64(15 - (2 ** 64 - 5)) == 20  # the difference is taken mod 2^64
    bad = R.Log(4, valid=False)
    bad.append([D.SENT_FIRST], [1], 2)
    assert bad.header() == {"capacity": 4, "count": 0, "dropped": 0}


# ------------------------------------------------------------------------------------------
# the report
# ------------------------------------------------------------------------------------------
def check_against_example(lats):
    ex = example_latency_report({b"c%d" % i: v for i, v in enumerate(lats)})
    rep = R.report(lats)
    assert rep["count"] == ex["total"]
    assert list(rep["pct_value"]) == ex["pct"]
    assert R.average(rep) == ex["average"]
    assert list(rep["sorted"][::-1]) == ex["rows"]  # the descending row list is the order read from the end
    assert [lats[j] for j in rep["order"]] == list(rep["sorted"])
    return rep


def test_thousand_samples_p999_reads_the_last_one():
    rng = np.random.default_rng(3)
    lats = [int(v) for v in rng.permutation(1000) * 3 + 7]  # distinct
    rep = check_against_example(lats)
    assert list(rep["pct_index"]) == [749, 799, 899, 949, 989, 999, 999]
    assert rep["pct_value"][5] == rep["sorted"][999] and rep["sorted"][998] != rep["sorted"][999]
    # 99.9 / 100.0 * 1000.0 is just above 999: not the textbook index 998
    assert (99.9 / 100.0) * 1000.0 > 999.0
    for n, idx in ((2000, 1998), (10000, 9990), (100000, 99900), (10 ** 6, 999000)):
        assert R.percentile_index(99.9, n) == idx


def test_one_sample_is_every_percentile():
    rep = check_against_example([-42])
    assert list(rep["pct_value"]) == [-42] * 7 and list(rep["pct_index"]) == [0] * 7
    assert list(rep["stats"]) == [-42, -42, -42] and R.average(rep) == -42.0
    r = R.report([5], pcts=(0.0, 100.0, 99.99))
    assert list(r["pct_index"]) == [0, 0, 0]


def test_negative_and_tied_latencies_keep_log_order():
    lats = [3, -1, 3, 0, -1, 3, R.INT64_MIN, R.INT64_MAX, -1]
    rep = check_against_example(lats)
    assert list(rep["order"]) == [6, 1, 4, 8, 3, 0, 2, 5, 7]
    assert list(rep["stats"]) == [sum(lats), R.INT64_MIN, R.INT64_MAX]
    wrap = R.report([R.INT64_MAX, R.INT64_MAX, 5])
    assert int(wrap["stats"][0]) == R.s64(2 * R.INT64_MAX + 5) == 3  # the sum is taken mod 2^64
    empty = R.report([])
    assert empty["count"] == 0 and list(empty["stats"]) == [0, 0, 0] and list(empty["pct_value"]) == [0] * 7
    assert list(empty["pct_index"]) == [0] * 7 and R.average(empty) == 0.0
    assert list(R.report(list(range(10)), pcts=(0.0, 100.0, 50.0))["pct_index"]) == [0, 9, 4]
