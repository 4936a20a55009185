"""The sequential models of the delivery reports (sbe_inflight_list_keys, sbe_latency_append,
sbe_latency_report) and the helpers of their tests.

list_keys works on delivery_lib.Table dicts: Python's sorted() on bytes is the order of
std::string::compare (bytes as unsigned, a proper prefix first).  Log is the latency log as a
list of (lat, tag); report() restates printLatencyReport's numbers
(examples/pubsub_reconnect_test.cpp:276-353) with its rank formula in Python floats, which are
IEEE doubles as the example's are."""
import math

import numpy as np

import delivery_lib as D

LIST_MAX = 64
LIST_IN_OTHER, LIST_NOT_IN_OTHER, LIST_ANSWERED, LIST_UNANSWERED = 1, 2, 4, 8
LAT_MAX_PCT = 16
REPORT_PERCENTILES = (75.0, 80.0, 90.0, 95.0, 99.0, 99.9, 99.99)
M64 = 2 ** 64 - 1
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1


def s64(x: int) -> int:
    """x mod 2^64 as a signed 64-bit value."""
    x &= M64
    return x - 2 ** 64 if x >= 2 ** 63 else x


def cdiv(a: int, b: int) -> int:
    """C++ integer division: truncation toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def slot_hash(key: bytes) -> int:
    """inf_hash of csrc/inflight.hpp: a key's chain in a table of `capacity` slots starts at
    slot_hash(key) & (capacity - 1)."""
    h = ((len(key) + 1) * 0xD6E8FEB86659FD93) & M64
    for j in range(5):
        h = ((h ^ int.from_bytes(key[8 * j: 8 * j + 8].ljust(8, b"\0"), "little")) * 0x9E3779B97F4A7C15) & M64
        h ^= h >> 29
    h = (h * 0xBF58476D1CE4E5B9) & M64
    return h ^ (h >> 32)


def random_keys(count, seed, lo=0, hi=40):
    """Distinct keys of lengths lo..hi with random bytes, zero bytes and shared prefixes among them."""
    rng = np.random.default_rng(seed)
    keys = set()
    while len(keys) < count:
        k = bytes(rng.integers(0, 256, int(rng.integers(lo, hi + 1)), dtype=np.uint8))
        keys.add(k)
        if len(k) < hi and rng.integers(0, 8) == 0:
            keys.add(k + b"\0")  # differs from k in the length alone
    return sorted(keys)[:count]


def keys_in_slot_range(count, seed, capacity, first, width):
    """Distinct keys whose chains all start in [first, first + width) of a `capacity`-slot table."""
    rng = np.random.default_rng(seed)
    keys = set()
    while len(keys) < count:
        k = b"n%x" % int(rng.integers(0, 2 ** 62))
        if first <= (slot_hash(k) & (capacity - 1)) < first + width:
            keys.add(k)
    return sorted(keys)


def list_keys(table, other=None, flags=0, min_value=0, limit=10):
    """-> (count, rows): every live entry of `table` (a delivery_lib.Table, or None for a table
    without a valid header) that passes, and the first `limit` as (key, value, answered) in key order."""
    live = {} if table is None else table.inflight
    answered = set() if table is None else table.answered
    members = None
    if flags & (LIST_IN_OTHER | LIST_NOT_IN_OTHER):
        members = set() if other is None else set(other.inflight)
    rows = []
    for k in sorted(live):
        v = live[k] & M64
        if members is not None and (k in members) != bool(flags & LIST_IN_OTHER):
            continue
        if flags & LIST_ANSWERED and k not in answered:
            continue
        if flags & LIST_UNANSWERED and k in answered:
            continue
        if v < min_value:
            continue
        rows.append((k, v, k in answered))
    return len(rows), rows[:limit]


class Log:
    """The latency log: samples in append order, at most `capacity` of them."""

    def __init__(self, capacity, valid=True):
        self.capacity, self.samples, self.dropped, self.valid = capacity, [], 0, valid

    def header(self):
        return {"capacity": self.capacity, "count": len(self.samples), "dropped": self.dropped}

    def append(self, code, value, now_ns, unit_ns=1_000_000, tag_base=0):
        if not self.valid:
            return
        for i, (c, v) in enumerate(zip(code, value)):
            if int(c) != D.SENT_FIRST:
                continue
            if len(self.samples) >= self.capacity:
                self.dropped += 1
                continue
            self.samples.append((cdiv(s64(int(now_ns) - int(v)), int(unit_ns)), (int(tag_base) + i) & M64))

    def lats(self):
        return [s[0] for s in self.samples]


def percentile_index(pct: float, count: int) -> int:
    """:322-326, operation for operation."""
    rank = (pct / 100.0) * float(count)
    idx = 0 if rank <= 0.0 else int(math.ceil(rank)) - 1
    return min(idx, count - 1)


def report(lats, pcts=REPORT_PERCENTILES):
    """What sbe_latency_report writes for the samples `lats` (log order)."""
    lats = [int(v) for v in lats]
    n = len(lats)
    order = sorted(range(n), key=lambda j: (lats[j], j))  # stable: ties in log order
    srt = [lats[j] for j in order]
    idx = [percentile_index(p, n) if n else 0 for p in pcts]
    return {"count": n,
            "stats": np.array([s64(sum(lats)), srt[0] if n else 0, srt[-1] if n else 0], np.int64),
            "pct_value": np.array([srt[i] if n else 0 for i in idx], np.int64),
            "pct_index": np.array(idx, np.uint64),
            "sorted": np.array(srt, np.int64), "order": np.array(order, np.uint32)}


def average(rep) -> float:
    """:334 on the host: (double)sum / (double)count."""
    return float(int(rep["stats"][0])) / float(rep["count"]) if rep["count"] else 0.0
