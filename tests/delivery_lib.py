"""The sequential models of delivery tracking and the generators of its tests.

Callback transcribes the second half of the subscriber's callback, examples/pubsub_reconnect_test.cpp:
625-691, and the publisher's two inserts (:455-459, :498-501) with Python sets and dicts.  Table
is the device table of sbe_inflight_* as a dict: inflight_lib.Model with the answered state, the
test-and-insert that counts (sbe_inflight_note_keys) and the lookup that marks on first sight
(sbe_inflight_lookup_keys); key_max as there.  expected_keys restates the rule of
sbe_delivery_keys over the outputs of the JSON reference of tests/jsonpaths_lib.py."""
import numpy as np

import inflight_lib as I
import jsonpaths_lib as J
import sbe_testlib as T

DLV_NONE, DLV_NEW, DLV_AGAIN, DLV_LONG, DLV_FULL = range(5)
SENT_NONE, SENT_UNKNOWN, SENT_FIRST, SENT_REPEAT, SENT_LONG = range(5)
NO_KEY = 0xFFFFFFFF
KEY_MAX = I.KEY_MAX
RECONNECT_THRESHOLD = 5  # DUPLICATE_DELIVERY_RECONNECT_THRESHOLD
KEY_FIELDS = ("msg_pos", "msg_len", "coid_pos", "coid_len", "coid_kind", "oid_pos", "oid_len", "oid_kind", "selected")


class Table(I.Model):
    """One device table.  self.inflight maps a live key to its 8-byte value."""

    def __init__(self, key_max=KEY_MAX):
        super().__init__(key_max)
        self.answered = set()
        self.seen.update(again_in_call=0, again_live=0, first_then_repeat=0, repeat_across=0, long=0, count5=0)

    def header(self, capacity):
        return {"capacity": capacity, "live": self.live, "used": self.used, "answered": len(self.answered)}

    def on_ack(self, message_id, timestamp_nanos):
        ok, base = super().on_ack(message_id, timestamp_nanos)
        if ok:
            self.answered.discard(message_id)  # the entry is erased with its mark
        return ok, base

    def note(self, keys):
        """keys[i]: bytes, or None (SBE_NO_KEY) -> code [n], count [n], totals [2]."""
        n = len(keys)
        code, count = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        first = set()
        for i, k in enumerate(keys):
            if k is None:
                continue
            k = bytes(k)
            if self.key_max is not None and len(k) > self.key_max:
                code[i] = DLV_LONG
                self.seen["long"] += 1
                continue
            if k in self.inflight:
                code[i] = DLV_AGAIN
                self.seen["again_in_call" if k in first else "again_live"] += 1
            else:
                code[i] = DLV_NEW
                self.inflight[k] = 0
                first.add(k)
                self.used += 1
            self.inflight[k] = (self.inflight[k] + 1) & (2 ** 64 - 1)
        for i, k in enumerate(keys):  # the count is the one the table holds after the whole call
            if code[i] in (DLV_NEW, DLV_AGAIN):
                count[i] = (self.inflight[bytes(k)] - 1) & 0xFFFFFFFF
                self.seen["count5"] += int(count[i]) == RECONNECT_THRESHOLD
        return code, count, np.array([(code == DLV_NEW).sum(), (code == DLV_AGAIN).sum()], np.uint64)

    def lookup(self, keys):
        """-> code [n], value [n], totals [3]."""
        n = len(keys)
        code, value = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
        first = set()
        for i, k in enumerate(keys):
            if k is None:
                continue
            k = bytes(k)
            if self.key_max is not None and len(k) > self.key_max:
                code[i] = SENT_LONG
            elif k not in self.inflight:
                code[i] = SENT_UNKNOWN
            elif k in self.answered:
                code[i] = SENT_REPEAT
                self.seen["first_then_repeat" if k in first else "repeat_across"] += 1
            else:
                code[i], value[i] = SENT_FIRST, self.inflight[k]
                self.answered.add(k)
                first.add(k)
        totals = [(code == SENT_FIRST).sum(), (code == SENT_REPEAT).sum(),
                  ((code == SENT_UNKNOWN) | (code == SENT_LONG)).sum()]
        return code, value, np.array(totals, np.uint64)

    def reset_values(self):
        for k in self.inflight:  # one delivery, no redelivery
            self.inflight[k] = 1

    def rehash(self):
        self.used = self.live


class Callback:
    """The tables of the example and what its callback does with one selected record."""

    def __init__(self):
        self.received_message_ids = set()
        self.duplicate_delivery_counts = {}
        self.received_client_order_ids = set()
        self.duplicate_client_order_ids = set()
        self.sent_client_order_ids = set()
        self.client_order_send_time = {}
        self.client_order_latency = {}
        self.messages_received = 0

    def publish(self, client_order_id, now):  # :455-459, :498-501
        self.sent_client_order_ids.add(client_order_id)
        self.client_order_send_time[client_order_id] = now

    def clear_duplicate_tracking(self):  # :70-73
        self.duplicate_delivery_counts.clear()

    def on_message(self, message_id, client_order_id, order_id, now):  # :625-691
        r = dict(already_processed=False, redeliveries=0, duplicate_client_order=False, was_sent=False,
                 latency_recorded=False, latency=0)
        if message_id:
            if message_id not in self.received_message_ids:
                self.received_message_ids.add(message_id)
                self.duplicate_delivery_counts.pop(message_id, None)  # note_successful_delivery
            else:
                r["already_processed"] = True
        if not r["already_processed"]:
            self.messages_received += 1
        if r["already_processed"]:
            c = self.duplicate_delivery_counts.get(message_id, 0) + 1  # record_duplicate_delivery
            self.duplicate_delivery_counts[message_id] = c
            r["redeliveries"] = c
            if client_order_id:
                self.received_client_order_ids.add(client_order_id)
        elif client_order_id:
            if client_order_id in self.received_client_order_ids:
                self.duplicate_client_order_ids.add(client_order_id)
                r["duplicate_client_order"] = True
            self.received_client_order_ids.add(client_order_id)
        if client_order_id:
            r["was_sent"] = client_order_id in self.sent_client_order_ids
            if client_order_id in self.client_order_send_time and client_order_id not in self.client_order_latency:
                r["latency_recorded"] = True
                r["latency"] = now - self.client_order_send_time[client_order_id]
                self.client_order_latency[client_order_id] = r["latency"]
        return r

    def missing(self):  # printMessageComparison: sent and never received
        return self.sent_client_order_ids - self.received_client_order_ids

    def extra(self):
        return self.received_client_order_ids - self.sent_client_order_ids


# ------------------------------------------------------------------------------------------
# keys as ranges of a buffer
# ------------------------------------------------------------------------------------------
def pack_ranges(keys, lead=3, tail=0):
    """(buf, key_pos u64, key_len u32): the keys back to back behind `lead` bytes, one filler byte
    between them, `tail` filler bytes behind the last (0: the last key ends with the buffer);
    None is SBE_NO_KEY at a position past the buffer."""
    pos, parts, at = [], [b"\xEE" * lead], lead
    last = max((i for i, k in enumerate(keys) if k is not None), default=-1)
    for i, k in enumerate(keys):
        if k is None:
            pos.append(2 ** 40 + i)
            continue
        pos.append(at)
        parts.append(bytes(k) + (b"\xEE" if i != last else b""))
        at += len(k) + (i != last)
    buf = np.frombuffer(b"".join(parts) + b"\xEE" * tail, np.uint8).copy()
    ln = np.array([NO_KEY if k is None else len(k) for k in keys], np.uint32)
    return buf, np.array(pos, np.uint64), ln


def clamped(buf_bytes, pos, ln):
    """The (pos, len) sbe_inflight_note_keys / _lookup_keys read for a range, after the clamp."""
    p = min(int(pos), buf_bytes)
    return p, min(int(ln), buf_bytes - p)


def keys_of(buf, pos, ln, buf_bytes=None):
    """The model's keys of a (buf, key_pos, key_len) triple: bytes per record, None for SBE_NO_KEY."""
    raw = bytes(np.asarray(buf, np.uint8))
    nb = len(raw) if buf_bytes is None else buf_bytes
    out = []
    for p, l in zip(pos, ln):
        if int(l) == NO_KEY:
            out.append(None)
            continue
        p, l = clamped(nb, p, l)
        out.append(raw[p: p + l])
    return out


# ------------------------------------------------------------------------------------------
# the rule of sbe_delivery_keys over the reference's extract (examples/pubsub_reconnect_test.cpp:592-619)
# ------------------------------------------------------------------------------------------
def expected_keys(rec_off, dec, select, ids):
    """Every output array of sbe_delivery_keys: dec the oracle's parse-mode decode, ids the
    reference extract over J.ORDER_ID_PATHS (view 3)."""
    n = len(rec_off) - 1
    out = {k: np.zeros(n, np.uint64 if k.endswith("pos") else np.uint32 if k.endswith("len") else np.uint8)
           for k in KEY_FIELDS}
    esc = 0
    for i in range(n):
        b, L = int(rec_off[i]), int(rec_off[i + 1]) - int(rec_off[i])

        def clamp(o, l):
            o = min(int(o), L)
            return o, min(int(l), L - o)

        sel = int(dec["status"][i]) == T.ST_TM and (select is None or bool(select[i]))
        out["selected"][i] = sel
        msg = client = order = (J.MISSING, 0, 0)
        if sel:
            msg = (J.STR,) + clamp(dec["view_off"][i][2], dec["view_len"][i][2])
            if ids["doc"][i] == J.OK and ids["root_kind"][i] == J.OBJ:
                kind = ids["kind"][i]

                def find_str(p):
                    if kind[p] not in (J.STR, J.ESC):
                        return (J.MISSING, 0, 0)
                    return (int(kind[p]),) + clamp(ids["off"][i][p], ids["len"][i][p])

                if kind[0] == J.OBJ and kind[1] == J.OBJ:
                    client, order = find_str(2), find_str(3)
                    # a string with bytes between its quotes decodes to a non-empty string, escaped or not
                    if client[2] == 0 and kind[4] == J.OBJ:
                        client = find_str(5)
                elif kind[0] == J.OBJ and kind[6] == J.OBJ:
                    client = find_str(7)
                if order[2] == 0 and find_str(8)[2]:
                    order = find_str(8)
        for name, (k, o, l) in (("msg", msg), ("coid", client), ("oid", order)):
            out[name + "_pos"][i] = b + o if l else b
            out[name + "_len"][i] = l if l else NO_KEY
            if name != "msg":
                out[name + "_kind"][i] = k
                esc += k == J.ESC
    out["totals"] = np.array([int(out["selected"].sum()), esc], np.uint64)
    return out


def strings_of(data, keys, i):
    """(message_id, client_order_id, order_id) of record i as the callback holds them: decoded."""
    raw = bytes(np.asarray(data, np.uint8))
    res = []
    for name in ("msg", "coid", "oid"):
        l = int(keys[name + "_len"][i])
        if l == NO_KEY:
            res.append(b"")
            continue
        tok = raw[int(keys[name + "_pos"][i]):][:l]
        res.append(J.unescape(tok) if name != "msg" and keys[name + "_kind"][i] == J.ESC else tok)
    return tuple(res)


def patch_escaped(data, keys):
    """What the host does when totals[1] != 0: the decoded bytes of every escaped client_order_id
    behind the batch, and coid_pos / coid_len pointing there.  Returns (buffer, coid_pos, coid_len)."""
    raw = bytearray(bytes(np.asarray(data, np.uint8)))
    pos, ln = keys["coid_pos"].copy(), keys["coid_len"].copy()
    for i in np.nonzero((keys["coid_kind"] == J.ESC) & (ln != NO_KEY))[0]:
        s = J.unescape(bytes(raw[int(pos[i]):][:int(ln[i])]))
        pos[i], ln[i] = len(raw), len(s)
        raw += s
    return np.frombuffer(bytes(raw), np.uint8).copy(), pos, ln


# ------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------
def _q(s: bytes) -> bytes:
    return b'"' + s + b'"'


def escaped(s: bytes) -> bytes:
    """s with its last byte spelled \\u00XX: another token, the same string."""
    return s[:-1] + b"\\u%04x" % s[-1]


FORMATS = ("inner", "details", "details_empty", "older", "uuid", "escaped", "esc_stop", "non_string", "non_object",
           "broken", "empty", "no_ids")


def payload(fmt, coid: bytes, oid: bytes) -> bytes:
    """A payload of one of FORMATS; coid / oid are plain ASCII without quotes or backslashes."""
    c, o = _q(coid), _q(oid)
    if fmt == "inner":  # message.message.client_order_id / order_id
        return b'{"message":{"message":{"client_order_id":%s,"order_id":%s,"qty":1}},"uuid":"not-this"}' % (c, o)
    if fmt == "details":  # no client_order_id in inner: falls through to order_details
        return b'{"message":{"message":{"order_id":%s,"order_details":{"client_order_id":%s}}}}' % (o, c)
    if fmt == "details_empty":  # an empty one falls through too
        return b'{"message":{"message":{"client_order_id":"","order_details":{"client_order_id":%s},"order_id":%s}}}' % (c, o)
    if fmt == "older":  # message.order_details, no order id anywhere
        return b'{"message":{"order_details":{"client_order_id":%s}}}' % c
    if fmt == "uuid":  # order id from the top-level uuid
        return b'{"uuid":%s,"message":{"message":{"client_order_id":%s,"order_id":""}}}' % (o, c)
    if fmt == "escaped":  # equal to the plain id after decodeString
        return b'{"message":{"message":{"client_order_id":%s,"order_id":%s}}}' % (_q(escaped(coid)), _q(escaped(oid)))
    if fmt == "esc_stop":  # a non-empty escaped id at path 2 stops the fall-through
        return b'{"message":{"message":{"client_order_id":%s,"order_details":{"client_order_id":"other"},"order_id":%s}}}' % (
            _q(escaped(coid)), o)
    if fmt == "non_string":  # only strings count
        return b'{"message":{"message":{"client_order_id":12345,"order_id":{"x":%s}}}}' % o
    if fmt == "non_object":
        return b'[%s,%s]' % (c, o)
    if fmt == "broken":
        return b'{"message":{"message":{"client_order_id":%s' % c
    if fmt == "empty":
        return b""
    return b'{"message":{"text":"hello"}}'  # no_ids


def has_ids(fmt):
    """(the callback finds a client_order_id, an order_id) in payload(fmt, ...)."""
    return (fmt in ("inner", "details", "details_empty", "older", "uuid", "escaped", "esc_stop"),
            fmt in ("inner", "details", "details_empty", "uuid", "escaped", "esc_stop"))


def order_record(message_id: bytes, fmt, coid: bytes, oid: bytes, ts=1):
    return T.tm_wire([b"order_notification_topic", b"CREATE_ORDER", bytes(message_id), payload(fmt, coid, oid), b"{}"], ts)


def client_ids(count, seed):
    """Distinct client order ids: uuid-like ones, the edge lengths 1, 39, 40 and 41 and longer ones,
    and families that differ in the last byte or in length."""
    rng = np.random.default_rng(seed)
    pool = [b"c", b"d", b"y" * 39, b"y" * 40, b"y" * 41, b"y" * 39 + b"z", b"z" * 60, b"ord-1", b"ord-2", b"ord-", b"ord-10"]
    while len(pool) < count:
        k = b"%08x-%04x-4%03x-%012x" % tuple(int(v) for v in rng.integers(0, [2 ** 32, 2 ** 16, 2 ** 12, 2 ** 48]))
        if rng.integers(0, 12) == 0:
            k = k + b"-long-suffix"  # 48 bytes
        if k not in pool:
            pool.append(k)
    return pool


def delivery_batch(seed, n, coids, first_msg=0, prior=()):
    """About n wire records and their select mask.  New order messages over `coids` in every
    format, redeliveries of `prior` (records of an earlier batch) and of this batch's own,
    two messages for one client_order_id, empty and long message ids, acks, undecodable records
    and unselected order messages.  Returns (records, select uint8)."""
    rng = np.random.default_rng(seed)
    recs, sel, mine = [], [], []
    prior = list(prior)
    for j in range(n):
        r = int(rng.integers(0, 40))
        if r == 0:
            recs.append(T.ack_wire(b"ack%d" % j, b"orders", b"c", 5 + j))
        elif r == 1:
            recs.append([b"", b"\x01\x02\x03", T.hdr_bytes(8, 9, 1, 1) + b"\0" * 12][j % 3])
        elif r < 8 and prior:  # a redelivery across batches
            recs.append(prior[int(rng.integers(0, len(prior)))])
        elif r < 14 and mine:  # ... and inside one; a hot head so that some come five times and more
            recs.append(mine[int(rng.integers(0, min(len(mine), 3 if r < 11 else len(mine))))])
        else:
            fmt = FORMATS[int(rng.integers(0, len(FORMATS)))] if r < 30 else "inner"
            coid = coids[int(rng.integers(0, len(coids)))]
            mid = b"msg_%d_%d" % (1_760_000_000_000_000 + seed, first_msg + j)
            if r == 14:
                mid = b""
            elif r == 15:
                mid = mid + b"_" + b"x" * 30  # over the key limit
            rec = order_record(mid, fmt, coid, b"oid-" + coid[:20], 100 + j)
            recs.append(rec)
            if mid:
                mine.append(rec)
        sel.append(0 if r == 39 else 1)
    return recs, np.array(sel, np.uint8)


def parsed(recs, select):
    """(data, rec_off, oracle decode, reference extract over the nine paths, expected keys)."""
    data, off = T.pack_records(recs)
    dec = T.oracle_decode(data, off, T.DEC_PARSE)
    ids = J.ref_extract(data, off, dec, J.ORDER_ID_PATHS, select=select)
    return data, off, dec, ids, expected_keys(off, dec, select, ids)


def random_ops(seed, calls=20, pool_size=400, max_records=300):
    """("remember", keys, ts) / ("note", keys) / ("lookup", keys) / ("reset",) / ("rehash",) calls over
    one key pool (inflight_lib.key_pool: every edge length); keys hold None for records without one."""
    rng = np.random.default_rng(seed)
    pool = I.key_pool(pool_size, seed + 1)
    ops = []
    for c in range(calls):
        n = int(rng.integers(max_records // 2, max_records + 1))
        idx = rng.integers(0, pool_size, n)
        idx[n // 2:] = rng.integers(0, 40, n - n // 2) + 40 * (c % 4)  # a hot range: repeats inside a call
        idx[: n // 10] = 7  # one key many times: its count passes five
        keys = [None if rng.integers(0, 12) == 0 else pool[i] for i in idx]
        kind = ("remember", "note", "lookup", "note", "lookup", "note", "reset", "lookup", "rehash", "note")[c % 10]
        if kind == "remember":
            ops.append((kind, [k if k is not None else b"" for k in keys], rng.integers(1, 2 ** 63, n, dtype=np.uint64)))
        elif kind in ("note", "lookup"):
            ops.append((kind, keys))
        else:
            ops.append((kind,))
    return pool, ops
