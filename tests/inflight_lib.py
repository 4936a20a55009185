"""The sequential model of ack correlation and the generators of its tests.

Model transcribes ClusterClient::remember_outgoing and on_ack_default (src/cluster_client.cpp:
1920-1941): inflight_ is a dict, emplace is setdefault, a match pops.  With key_max set it also
reports what the device table reports about keys it cannot hold (sbe_inflight_* of
include/sbecodec.h), and counts `live` / `used` as the table's header does."""
import numpy as np

import sbe_testlib as T

INF_INSERTED, INF_DUPLICATE, INF_SKIPPED, INF_KEY_TOO_LONG, INF_FULL = range(5)
ACK_NONE, ACK_MATCHED, ACK_UNMATCHED, ACK_LONG_ID = range(4)
KEY_MAX = 40
EDGE_LENS = (0, 1, 39, 40, 41)


class Model:
    def __init__(self, key_max=KEY_MAX):
        self.inflight = {}
        self.key_max = key_max
        self.used = 0  # inserts so far: erased slots are not reused
        self.erased = set()
        # what the random-sequence test wants to have seen
        self.seen = dict(dup_in_call=0, dup_live=0, reinsert=0, repeat_ack=0)

    @property
    def live(self):
        return len(self.inflight)

    def remember(self, keys, ts=None, ts_default=0, mask=None):
        """remember_outgoing(keys[i], ts[i]) for every i whose offer succeeded -> status [n]."""
        st = np.empty(len(keys), np.uint8)
        first = {}
        for i, k in enumerate(keys):
            k = bytes(k)
            if mask is not None and not mask[i]:
                st[i] = INF_SKIPPED
                continue
            if self.key_max is not None and len(k) > self.key_max:
                st[i] = INF_KEY_TOO_LONG
                continue
            t = int(ts[i]) if ts is not None else 0
            t = t if t else int(ts_default)
            if k in self.inflight:
                st[i] = INF_DUPLICATE
                self.seen["dup_in_call" if k in first else "dup_live"] += 1
                continue
            self.inflight.setdefault(k, t)  # inflight_.emplace(uuid, ts_nanos)
            first[k] = i
            self.used += 1
            if k in self.erased:
                self.erased.discard(k)
                self.seen["reinsert"] += 1
            st[i] = INF_INSERTED
        return st

    def on_ack(self, message_id, timestamp_nanos):
        """on_ack_default -> (matched, the time it subtracts from now_nanos())."""
        if message_id and message_id in self.inflight:
            self.erased.add(message_id)
            return True, self.inflight.pop(message_id)
        return False, int(timestamp_nanos)

    def match(self, acks):
        """acks: (egress status, message_id, timestamp_nanos) per record -> code, base_ns, counts."""
        code = np.empty(len(acks), np.uint8)
        base = np.zeros(len(acks), np.uint64)
        ids = set()
        for i, (st, mid, ts) in enumerate(acks):
            if st not in (T.ST_EG_ACK, T.ST_EG_ACK_SIMPLE):
                code[i] = ACK_NONE
                continue
            mid = bytes(mid)
            if mid:
                self.seen["repeat_ack"] += mid in ids
                ids.add(mid)
            if self.key_max is not None and len(mid) > self.key_max:
                code[i], base[i] = ACK_LONG_ID, ts
                continue
            ok, b = self.on_ack(mid, ts)
            code[i], base[i] = (ACK_MATCHED if ok else ACK_UNMATCHED), b
        counts = np.array([(code == ACK_MATCHED).sum(), ((code == ACK_UNMATCHED) | (code == ACK_LONG_ID)).sum()],
                          np.uint64)
        return code, base, counts


def acks_of(data, off, dec):
    """The model's view of an on-egress decode: (status, message_id, timestamp_nanos) per record."""
    out = []
    raw = bytes(np.asarray(data, np.uint8))
    for i in range(len(off) - 1):
        st = int(dec["status"][i])
        mid = b""
        if st == T.ST_EG_ACK:
            b = int(off[i]) + int(dec["view_off"][i][0])
            mid = raw[b: b + int(dec["view_len"][i][0])]
        out.append((st, mid, int(dec["ts"][i])))
    return out


def pack_keys(keys, lead=3):
    """(arena, key_off, key_len): the keys back to back behind `lead` bytes, one filler byte between
    them, so that no key is aligned and a read past a key's end picks up foreign bytes."""
    off, parts, pos = [], [b"\xEE" * lead], lead
    for k in keys:
        off.append(pos)
        parts.append(bytes(k) + b"\xEE")
        pos += len(k) + 1
    arena = np.frombuffer(b"".join(parts) + b"\xEE" * 8, np.uint8).copy()
    return arena, np.array(off, np.uint32), np.array([len(k) for k in keys], np.uint32)


def key_pool(count, seed):
    """Distinct keys: "pub_<nanos>" uuids as publish_topic makes them, keys of the edge lengths
    0, 1, 39, 40, 41, and families that differ only in the last byte, the length or zero padding."""
    rng = np.random.default_rng(seed)
    pool = [b"", b"a", b"a\0", b"a\0\0", b"b", b"x" * 39, b"x" * 40, b"x" * 41, b"x" * 39 + b"y", b"y" * 41,
            b"x" * 38 + b"\0", b"pub_1760000000000000000", b"pub_1760000000000000001", b"pub_176000000000000000"]
    base = 1_760_000_000_000_000_000
    while len(pool) < count:
        r = int(rng.integers(0, 10))
        if r == 0:
            k = bytes(rng.integers(0, 256, int(rng.choice(EDGE_LENS[1:])), dtype=np.uint8))
        elif r == 1:
            k = bytes(rng.integers(0, 256, int(rng.integers(1, 48)), dtype=np.uint8))
        else:
            k = b"pub_%d" % (base + int(rng.integers(0, 5000)))
        if k not in pool:
            pool.append(k)
    return pool


def full_ack(message_id, topic, corr, ts):
    """A full ack as decode_ack accepts it: the reference wraps the flyweight with len - 8
    (src/ack_decoder.cpp:67), so the record needs eight more bytes than its fields take."""
    return T.ack_wire(bytes(message_id), topic, corr, ts) + b"\0" * 8


def ack_records(rng, ids, ts0):
    """Wire records for a match call: a full ack per id, with simple acks, TopicMessages, acks with
    an empty id and undecodable records mixed in."""
    recs = []
    for j, k in enumerate(ids):
        r = int(rng.integers(0, 16))
        if r == 0:
            recs.append(T.simple_ack(ts0 + 1000 + j))
        elif r == 1:
            recs.append(T.tm_wire([b"orders", b"X", bytes(k)[:30], b"{}", b"{}"], ts0 + j) + b"\0" * 8)  # len - 8 again
        elif r == 2:
            recs.append([b"", b"\x01\x02\x03", T.hdr_bytes(8, 9, 1, 1) + b"\0" * 12][j % 3])
        elif r == 3:
            recs.append(full_ack(b"", b"orders", b"c", ts0 + j))
        recs.append(full_ack(k, b"orders", b"corr%d" % j, ts0 + 7 * j + 1))
    return recs


def random_ops(seed, calls=20, pool_size=400, max_records=300):
    """Alternating ("remember", keys, ts, mask) / ("match", records) calls over one key pool."""
    rng = np.random.default_rng(seed)
    pool = key_pool(pool_size, seed + 1)
    ops = []
    for c in range(calls):
        n = int(rng.integers(max_records // 2, max_records + 1))
        if c % 2 == 0:
            idx = rng.integers(0, pool_size, n)
            idx[n // 2:] = rng.integers(0, 60, n - n // 2) + 60 * (c % 5)  # a hot range: duplicates inside a call
            keys = [pool[i] for i in idx]
            ts = rng.integers(1, 2 ** 63, n, dtype=np.uint64)
            ts[::11] = 0
            mask = (rng.integers(0, 8, n) != 0).astype(np.uint8)
            ops.append(("remember", keys, ts, mask))
        else:
            idx = rng.integers(0, pool_size, n // 2)
            idx[: n // 8] = idx[n // 8: 2 * (n // 8)]  # the same id twice in one call
            rng.shuffle(idx)
            ops.append(("match", ack_records(rng, [pool[i] for i in idx], 1_760_000_000_000 + c)))
    return pool, ops
