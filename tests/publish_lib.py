"""Shared by the publish_orders tests: a Python restatement of Order::validate()
(src/order_types.cpp:66-120, :455-467), the hand table of orders, a seeded batch that mixes valid
orders with every kind of invalid one, the expected records (oracle JSON texts put through the
oracle encoder; never the code under test), the device front end and the build of tests/publish."""
import os
import subprocess

import numpy as np

import sbe_testlib as T

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "publish")

MESSAGES = ("Order ID is required", "Base token is required", "Quote token is required",
            "Side must be 'BUY' or 'SELL'", "Quantity must be positive", "Invalid order type: ",
            "Limit price must be positive for LIMIT orders", "Stop price must be positive for STOP orders",
            "Stop price must be positive for STOP_LIMIT orders", "Limit price must be positive for STOP_LIMIT orders",
            "Invalid time in force: ", "Expiry timestamp required for GTD orders")
INVALID_BASE = 16  # SBE_PUB_INVALID_ID
HAS_STOP, HAS_EXPIRY = 1, 2
E109_TOPIC, E109_UUID, E109_PAYLOAD, E109_HEADERS, OVERFLOW = 1, 3, 4, 5, 6
# field indices of sbe_order_batch
F_UUID, F_IDENT, F_BASE, F_QUOTE, F_SIDE, F_ID, F_MSGID, F_STATUS = range(8)


def binary(name):
    """Builds tests/publish/<name> on demand and returns its path."""
    subprocess.run(["make", "-s", "-C", DIR, name], check=True)
    return os.path.join(DIR, name)


def validate_mask(f, q, order_type, tif, limit_price, stop_price, present) -> int:
    """Bit k set iff validate() returns message k (in the reference's order)."""
    has_stop, has_expiry = bool(present & HAS_STOP), bool(present & HAS_EXPIRY)
    m = 0
    if len(f[F_ID]) == 0:                                        # :69
        m |= 1 << 0
    if len(f[F_BASE]) == 0:                                      # :73
        m |= 1 << 1
    if len(f[F_QUOTE]) == 0:                                     # :77
        m |= 1 << 2
    if f[F_SIDE] not in (b"BUY", b"SELL"):                       # :81, :455
        m |= 1 << 3
    if q <= 0.0:                                                 # :85 (false for NaN)
        m |= 1 << 4
    if order_type not in (b"MARKET", b"LIMIT", b"STOP", b"STOP_LIMIT"):  # :89, :459
        m |= 1 << 5
    if order_type == b"LIMIT" and limit_price <= 0.0:            # :94
        m |= 1 << 6
    stop_bad = (not has_stop) or stop_price <= 0.0
    if order_type == b"STOP" and stop_bad:                       # :98
        m |= 1 << 7
    if order_type == b"STOP_LIMIT":                              # :102
        if stop_bad:
            m |= 1 << 8
        if limit_price <= 0.0:
            m |= 1 << 9
    if tif not in (b"GTC", b"IOC", b"FOK", b"DAY", b"GTD"):      # :111, :464
        m |= 1 << 10
    if tif == b"GTD" and not has_expiry:                         # :115
        m |= 1 << 11
    return m


def first_status(mask: int) -> int:
    return 0 if mask == 0 else INVALID_BASE + (mask & -mask).bit_length() - 1


class Batch:
    """Host arrays of an Order batch plus its checks."""

    def __init__(self, fields, cid, ts, q, order_type, tif, limit_price, stop_price, present):
        self.fields = [list(f) for f in fields]
        self.n = len(fields)
        self.cid = np.asarray(cid, np.int64)
        self.ts = np.asarray(ts, np.int64)
        self.q = np.asarray(q, np.float64)
        self.order_type, self.tif = list(order_type), list(tif)
        self.limit_price = np.asarray(limit_price, np.float64)
        self.stop_price = np.asarray(stop_price, np.float64)
        self.present = np.asarray(present, np.uint8)

    def masks(self):
        return np.array([validate_mask(self.fields[i], float(self.q[i]), self.order_type[i], self.tif[i],
                                       float(self.limit_price[i]), float(self.stop_price[i]), int(self.present[i]))
                         for i in range(self.n)], np.uint16)


def _good(i):
    return dict(f=[b"uuid-%d" % i, b"ident", b"BTC", b"USDC", b"BUY", b"id-%d" % i, b"msg_1_%05d" % (10000 + i),
                   b"CREATED"], q=1.5, ot=b"LIMIT", tif=b"GTC", lim=10.0, stop=0.0, pres=0)


def hand_table():
    """(Batch, expected message lists): one order per message, then the issue's extra cases.  The
    texts are literal; the C++ mirror test and the device test share the rows."""
    rows, texts = [], []

    def add(expect, **kw):
        r = _good(len(rows))
        for k, v in kw.items():
            if isinstance(k, str) and k.startswith("f") and k[1:].isdigit():
                r["f"][int(k[1:])] = v
            else:
                r[k] = v
        rows.append(r)
        texts.append(expect)

    add(["Order ID is required"], f5=b"")
    add(["Base token is required"], f2=b"")
    add(["Quote token is required"], f3=b"")
    add(["Side must be 'BUY' or 'SELL'"], f4=b"HOLD")
    add(["Quantity must be positive"], q=-1.0)
    add(["Invalid order type: ICEBERG"], ot=b"ICEBERG")
    add(["Limit price must be positive for LIMIT orders"], lim=0.0)
    add(["Stop price must be positive for STOP orders"], ot=b"STOP")
    add(["Stop price must be positive for STOP_LIMIT orders"], ot=b"STOP_LIMIT")
    add(["Limit price must be positive for STOP_LIMIT orders"], ot=b"STOP_LIMIT", stop=5.0, pres=HAS_STOP, lim=-2.0)
    add(["Invalid time in force: GTX"], tif=b"GTX")
    add(["Expiry timestamp required for GTD orders"], tif=b"GTD")
    # STOP_LIMIT with both prices bad: two messages, in order
    add(["Stop price must be positive for STOP_LIMIT orders", "Limit price must be positive for STOP_LIMIT orders"],
        ot=b"STOP_LIMIT", stop=-1.0, pres=HAS_STOP, lim=0.0)
    add(["Expiry timestamp required for GTD orders"], tif=b"GTD", ot=b"MARKET")  # GTD without expiry
    add([], tif=b"GTD", pres=HAS_EXPIRY)
    add([], q=float("nan"))                                    # NaN <= 0.0 is false: passes
    add(["Quantity must be positive"], q=-0.0)                 # -0.0 <= 0.0 is true
    add(["Side must be 'BUY' or 'SELL'"], f4=b"buy")           # exact match only
    # an all-defaults Order: empty strings, quantity 0, LIMIT at limit_price 0, GTC
    add(["Order ID is required", "Base token is required", "Quote token is required",
         "Side must be 'BUY' or 'SELL'", "Quantity must be positive",
         "Limit price must be positive for LIMIT orders"],
        f0=b"", f1=b"", f2=b"", f3=b"", f4=b"", f5=b"", f7=b"", q=0.0, lim=0.0)
    add([], ot=b"STOP", stop=3.0, pres=HAS_STOP, f7=b"UPDATED")
    add([], ot=b"MARKET", lim=0.0, f4=b"SELL", f7=b"CANCELLED")
    b = Batch([r["f"] for r in rows], np.arange(len(rows)) + 7, 1_760_000_000_000_000_000 + np.arange(len(rows)),
              [r["q"] for r in rows], [r["ot"] for r in rows], [r["tif"] for r in rows], [r["lim"] for r in rows],
              [r["stop"] for r in rows], [r["pres"] for r in rows])
    return b, texts


def mixed_batch(n, seed):
    """T.order_batch(hard=True) strings with sides, quantities and checks drawn so that the batch
    mixes valid orders with every validation failure: order i has exactly defect i % 16 for
    0..11 (its status is that code), none for 12 and 13, two defects for 14, and is left as the
    generator drew it for 15 (usually several)."""
    fields, cid, ts, q = T.order_batch(n, seed, hard=True)
    rng = np.random.default_rng(seed + 1000)
    q = np.array(q, np.float64)
    ot, tif, lim, stop, pres = [], [], np.zeros(n), np.zeros(n), np.zeros(n, np.uint8)
    bad_q = [-1.0, 0.0, -0.0, float("-inf"), -5e-324]
    for i in range(n):
        f = fields[i]
        kind = i % 16
        o_t = [b"MARKET", b"LIMIT", b"STOP", b"STOP_LIMIT"][int(rng.integers(0, 4))]
        t_f = [b"GTC", b"IOC", b"FOK", b"DAY", b"GTD"][int(rng.integers(0, 5))]
        lim[i], stop[i] = float(rng.integers(1, 1000)) / 8, float(rng.integers(1, 1000)) / 4
        pres[i] = HAS_STOP | HAS_EXPIRY if rng.random() < 0.8 else (HAS_STOP if o_t in (b"STOP", b"STOP_LIMIT") else 0)
        if t_f == b"GTD":
            pres[i] |= HAS_EXPIRY
        if kind != 15:  # a valid order first
            f[F_SIDE] = b"BUY" if rng.random() < 0.5 else b"SELL"
            for j, dflt in ((F_ID, b"id%d" % i), (F_BASE, b"BTC"), (F_QUOTE, b"USDC")):
                if len(f[j]) == 0:
                    f[j] = dflt
            if not (q[i] > 0.0):
                q[i] = float("nan") if rng.random() < 0.2 else 1.5
        defects = [kind] if kind < 12 else ([int(x) for x in rng.choice(12, 2, replace=False)] if kind == 14 else [])
        for d in defects:
            if d == 0:
                f[F_ID] = b""
            elif d == 1:
                f[F_BASE] = b""
            elif d == 2:
                f[F_QUOTE] = b""
            elif d == 3:
                f[F_SIDE] = [b"buy", b"", b"BUY\x00", b"SELLX", b"BU"][int(rng.integers(0, 5))]
            elif d == 4:
                q[i] = bad_q[int(rng.integers(0, len(bad_q)))]
            elif d == 5:
                o_t = [b"limit", b"", b"LIMIT\x00", b"STOP_LIMI", b"MARKETS"][int(rng.integers(0, 5))]
            elif d == 6:
                o_t, lim[i] = b"LIMIT", [0.0, -1.0, -0.0][int(rng.integers(0, 3))]
            elif d == 7:
                o_t = b"STOP"
                if rng.random() < 0.5:
                    pres[i] &= ~np.uint8(HAS_STOP)
                else:
                    stop[i] = 0.0
            elif d == 8:
                o_t = b"STOP_LIMIT"
                if rng.random() < 0.5:
                    pres[i] &= ~np.uint8(HAS_STOP)
                else:
                    stop[i] = -2.5
            elif d == 9:
                o_t, lim[i] = b"STOP_LIMIT", 0.0
                if 8 not in defects:
                    pres[i] |= HAS_STOP
                    stop[i] = stop[i] if stop[i] > 0 else 1.0
            elif d == 10:
                t_f = [b"gtc", b"", b"GTC ", b"GT"][int(rng.integers(0, 4))]
            elif d == 11:
                t_f = b"GTD"
                pres[i] &= ~np.uint8(HAS_EXPIRY)
        ot.append(o_t)
        tif.append(t_f)
    return Batch(fields, cid, ts, q, ot, tif, lim, stop, pres)


def pack2(a, b):
    """Two strings per record → (packed arena uint8, str_len uint32 [n,2])."""
    flat = [s for pair in zip(a, b) for s in pair]
    arena = np.frombuffer(b"".join(flat), np.uint8) if flat else np.zeros(0, np.uint8)
    return arena, np.array([len(s) for s in flat], np.uint32).reshape(-1, 2)


def texts(b: Batch):
    arena, str_len = T.pack_order_fields(b.fields)
    pay, po = T.oracle_order_json(arena, str_len, b.cid, b.ts, b.q, 0, nthreads=8)
    hdr, ho = T.oracle_order_json(arena, str_len, b.cid, b.ts, b.q, 1, nthreads=8)
    return (pay, po.astype(np.int64)), (hdr, ho.astype(np.int64))


def expected(b: Batch, topic: bytes, tm_ts, ts_default, flags, session, term=0, sess=0, validate=True, txt=None):
    """(records list of bytes, out_off uint64 [n+1], status uint8 [n], mask uint16 [n]) with no
    capacity limit: oracle texts → 5-field arena → oracle encoder, for the orders validate() passes."""
    n = b.n
    (pay, po), (hdr, ho) = txt if txt is not None else texts(b)
    mask = b.masks() if validate else np.zeros(n, np.uint16)
    status = np.array([first_status(int(m)) for m in mask], np.uint8)
    keep = np.nonzero(mask == 0)[0]
    recs = [b""] * n
    if keep.size:
        types = b"CREATE_ORDERUPDATE_ORDER"
        ids = b"".join(b.fields[i][F_MSGID] for i in keep)
        b_types, b_ids = len(topic), len(topic) + len(types)
        b_pay = b_ids + len(ids)
        b_hdr = b_pay + len(pay)
        arena = np.frombuffer(topic + types + ids + pay + hdr, np.uint8)
        assert arena.size < 2 ** 32
        off = np.zeros((keep.size, 5), np.uint32)
        ln = np.zeros((keep.size, 5), np.uint32)
        at = 0
        for r, i in enumerate(keep):
            upd = b.fields[i][F_STATUS] in (b"UPDATED", b"CANCELLED")  # src/cluster_client.cpp:309-312
            idl = len(b.fields[i][F_MSGID])
            off[r] = (0, b_types + (12 if upd else 0), b_ids + at, b_pay + po[i], b_hdr + ho[i])
            ln[r] = (len(topic), 12, idl, po[i + 1] - po[i], ho[i + 1] - ho[i])
            at += idl
        ts = np.zeros(keep.size, np.uint64) if tm_ts is None else np.asarray(tm_ts, np.uint64)[keep]
        if session:
            eo, eoff, est = T.oracle_encode_session(arena, ln, ts, term, sess, str_off=off, flags=flags,
                                                    ts_default=ts_default, nthreads=8)
        else:
            eo, eoff, est = T.oracle_encode(arena, ln, ts, str_off=off, flags=flags, ts_default=ts_default, nthreads=8)
        eo = eo.tobytes()
        for r, i in enumerate(keep):
            recs[i] = eo[int(eoff[r]):int(eoff[r + 1])]
            status[i] = est[r]
    out_off = np.zeros(n + 1, np.uint64)
    out_off[1:] = np.cumsum([len(r) for r in recs])
    return recs, out_off, status, mask


def run_device(codec, b: Batch, topic: bytes, tm_ts=None, ts_default=0, flags=1, session=True, term=0, sess=0,
               validate=True, with_off=False, before_call=None, **kw):
    """→ (out uint8 array, out_off uint64, status, mask) of codec.publish_orders_batch.
    before_call(): run once every input is on the device and the device is idle, right before the call."""
    import torch
    n = b.n
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
    arena, str_len = T.pack_order_fields(b.fields)
    c_arena, c_len = pack2(b.order_type, b.tif)
    str_off = c_off = None
    if with_off:  # the same strings, record order reversed in the arenas; "orders" / "checks": that arena only
        pieces, offs, at = [], np.zeros((n, 8), np.uint32), 0
        cp, coffs, cat = [], np.zeros((n, 2), np.uint32), 0
        for i in reversed(range(n)):
            for j in range(8):
                offs[i, j] = at
                pieces.append(b.fields[i][j])
                at += len(b.fields[i][j])
            for j, s in enumerate((b.tif[i], b.order_type[i])):  # time_in_force first in the arena
                coffs[i, 1 - j] = cat
                cp.append(s)
                cat += len(s)
        if with_off in (True, "orders"):
            arena, str_off = np.frombuffer(b"".join(pieces), np.uint8), dev(offs, np.int32)
        if with_off in (True, "checks"):
            c_arena, c_off = np.frombuffer(b"".join(cp), np.uint8), dev(coffs, np.int32)
    one = lambda a: a if a.size else np.zeros(1, np.uint8)
    checks = None
    if validate:
        checks = (dev(one(c_arena), np.uint8), dev(c_len, np.int32), dev(b.limit_price, np.float64),
                  dev(b.stop_price, np.float64), dev(b.present, np.uint8)) + ((c_off,) if c_off is not None else ())
    args = (dev(one(arena), np.uint8), dev(str_len, np.int32), dev(b.cid, np.int64), dev(b.ts, np.int64),
            dev(b.q, np.float64), dev(np.frombuffer(topic, np.uint8), np.uint8))
    tm = None if tm_ts is None else dev(np.asarray(tm_ts, np.uint64).view(np.int64), np.int64)
    if before_call is not None:
        torch.cuda.synchronize()
        before_call()
    r = codec.publish_orders_batch(*args, checks=checks, str_off=str_off, tm_timestamp=tm, ts_default=ts_default,
                                   flags=flags, session=session, leadership_term_id=term, cluster_session_id=sess, **kw)
    if kw.get("stream") is not None:
        kw["stream"].synchronize()  # the results are complete once the call's own stream is
        got = (r.out.cpu().numpy(), r.out_off.cpu().numpy().view(np.uint64), r.status.cpu().numpy()[:n],
               r.error_mask.cpu().numpy().view(np.uint16)[:n])
        torch.cuda.synchronize()
        return got
    torch.cuda.synchronize()
    return (r.out.cpu().numpy(), r.out_off.cpu().numpy().view(np.uint64), r.status.cpu().numpy()[:n],
            r.error_mask.cpu().numpy().view(np.uint16)[:n])


def assert_records(got, exp, cap=None):
    """Every record's bytes, out_off, status and error_mask; with cap, records ending past it are
    SBE_ENC_OVERFLOW and unwritten."""
    out, off, st, mask = got
    recs, eoff, est, emask = exp
    assert np.array_equal(off, eoff)
    assert np.array_equal(mask, emask)
    est = est.copy()
    if cap is not None:
        over = (eoff[1:] > cap) & (np.diff(eoff.astype(np.int64)) > 0)
        est[over] = OVERFLOW
    bad = np.nonzero(st != est)[0]
    assert bad.size == 0, (bad[:5], st[bad[:5]], est[bad[:5]])
    data = out.tobytes()
    for i, r in enumerate(recs):
        if est[i] == 0:
            a = int(off[i])
            assert data[a:a + len(r)] == r, (i, data[a:a + len(r)][:120], r[:120])


# ---- the order file of tests/publish (order_file.hpp) ----
def write_orders(path, b: Batch, topic: bytes, tm_ts=None, session=True, truncate8=True, term=0, sess=0):
    import struct
    s = lambda x: struct.pack("<I", len(x)) + bytes(x)
    parts = [struct.pack("<IBBqq", b.n, int(session), int(truncate8), term, sess), s(topic)]
    for i in range(b.n):
        parts += [s(f) for f in b.fields[i]] + [s(b.order_type[i]), s(b.tif[i])]
        parts.append(struct.pack("<dqqddBQ", float(b.q[i]), int(b.cid[i]), int(b.ts[i]), float(b.limit_price[i]),
                                 float(b.stop_price[i]), int(b.present[i]), 0 if tm_ts is None else int(tm_ts[i])))
    with open(path, "wb") as f:
        f.write(b"".join(parts))


class Parse:
    def __init__(self, path):
        with open(path, "rb") as f:
            self.d, self.at = f.read(), 0

    def u32(self):
        self.at += 4
        return int.from_bytes(self.d[self.at - 4:self.at], "little")

    def take(self, n):
        self.at += n
        return self.d[self.at - n:self.at]

    def string(self):
        return self.take(self.u32())

    def done(self):
        return self.at == len(self.d)
