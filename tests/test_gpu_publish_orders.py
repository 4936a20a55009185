"""sbe_publish_orders_batch on the GPU: ClusterClient::publish_order (src/cluster_client.cpp:300-372)
for a batch, fused.  Every record's bytes, out_off, status and error_mask are compared with the
composition the reference performs: Order::validate() (restated in publish_lib.validate_mask), the
oracle's JSON texts, and the oracle's TopicMessage / session encoder over them.  Parity is bit-exact
against that oracle composition; against jsoncpp itself it is unpinned (jsoncpp absent), as for
tests/test_gpu_orderjson.py."""
import functools

import numpy as np
import pytest

import publish_lib as P
import sbe_testlib as T

TOPIC = b"orders"


@functools.lru_cache(maxsize=None)
def mixed(n):
    b = P.mixed_batch(n, 100 + n)
    return b, P.texts(b)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,session", [(0, False), (0, True), (1, False), (1, True)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099, 20000])
def test_parity(codec, n, flags, session):
    b, txt = mixed(n)
    tm_ts = np.arange(n, dtype=np.uint64) % 3 * 1_000_003  # every third record takes ts_default
    exp = P.expected(b, TOPIC, tm_ts, 424242, flags, session, term=-5, sess=2 ** 40 + 9, txt=txt)
    if n >= 63:  # the batch holds every validation code and valid records (n = 1 cannot)
        st = exp[2]
        assert set(range(16, 28)) <= set(st.tolist()) and (st == 0).sum() >= n // 16
        assert (np.array([bin(int(m)).count("1") for m in exp[3]]) >= 2).any()
    # both arenas packed, both through str_off, and the two mixed forms (each takes its own
    # branches in the totals and sizing launches)
    for with_off in (False, True, "orders", "checks"):
        got = P.run_device(codec, b, TOPIC, tm_ts, 424242, flags, session, term=-5, sess=2 ** 40 + 9,
                           with_off=with_off)
        P.assert_records(got, exp)
    strings = sum(len(x) for f in b.fields for x in f)
    assert int(exp[1][-1]) <= codec.publish_orders_output_bound(n, strings, len(TOPIC), session)


@pytest.mark.gpu
def test_validation_table(codec):
    b, texts = P.hand_table()
    mask = b.masks()
    for i, t in enumerate(texts):  # the restatement agrees with the literal table
        got = [P.MESSAGES[k] + (b.order_type[i].decode() if k == 5 else b.tif[i].decode() if k == 10 else "")
               for k in range(12) if int(mask[i]) >> k & 1]
        assert got == t, i
    exp = P.expected(b, TOPIC, None, 99, 1, True, 3, 4)
    assert set(exp[2].tolist()) >= set(range(16, 28))
    P.assert_records(P.run_device(codec, b, TOPIC, None, 99, 1, True, 3, 4), exp)
    # checks == NULL: the caller has validated, everything encodes
    exp = P.expected(b, TOPIC, None, 99, 1, True, 3, 4, validate=False)
    assert (exp[2] == 0).all() and (exp[3] == 0).all()
    P.assert_records(P.run_device(codec, b, TOPIC, None, 99, 1, True, 3, 4, validate=False), exp)


@pytest.mark.gpu
def test_size_classes(codec):
    """Ordinary records, records with a 600-byte control-character field (several window passes) and
    records over any LDS window (straight to HBM) in one batch; then with a capacity that cuts a
    large record, and a sentinel after the capacity that must survive."""
    import torch
    n = 1000
    b = P.mixed_batch(n, 31)
    for i, f in enumerate(b.fields):
        if i % 37 == 5:  # over any window: payload ~42 KB, headers ~63 KB; 7000 control bytes: E109_PAYLOAD
            j, k = ((P.F_UUID, 3500), (P.F_MSGID, 10500), (P.F_UUID, 7000))[i % 3]
            f[j] = b"\x01" * k
        elif i % 11 == 3:  # ~12 KB: a window pass of its own
            f[P.F_UUID] = f[P.F_MSGID] = b"\x02" * 600
    # checks == NULL, so that every size class is emitted whatever the drawn validity
    exp = P.expected(b, TOPIC, None, 5, 0, True, 1, 2, validate=False)
    sizes = np.diff(exp[1].astype(np.int64))
    assert sizes.max() > 60000 and (sizes > 40000).sum() >= 15 and (exp[2] == P.E109_PAYLOAD).sum() >= 5
    assert ((sizes > 8000) & (sizes < 20000)).sum() > 50 and ((sizes > 0) & (sizes < 2000)).sum() > 500
    P.assert_records(P.run_device(codec, b, TOPIC, None, 5, 0, True, 1, 2, validate=False), exp)
    # the a-priori bound holds where nearly every string byte escapes to six
    strings = sum(len(x) for f in b.fields for x in f)
    assert int(exp[1][-1]) <= codec.publish_orders_output_bound(n, strings, len(TOPIC), True)
    big = next(i for i in range(500, n) if sizes[i] > 40000)
    cap = int(exp[1][big]) + 1000  # ends inside a record that goes straight to HBM
    buf = torch.full((cap + 80000,), 0xAB, dtype=torch.uint8, device="cuda")
    got = P.run_device(codec, b, TOPIC, None, 5, 0, True, 1, 2, validate=False, out=buf, out_capacity=cap)
    P.assert_records(got, exp, cap=cap)
    assert (got[2] == P.OVERFLOW).sum() > 100
    assert (got[0][cap:] == 0xAB).all(), "write past out_capacity"


def _grow_to(b, i, field, what, target):
    """Grows the plain-ASCII `field` of order i until its text `what` is exactly `target` bytes."""
    one = lambda: len(T.oracle_order_json_one(b.fields[i], b.cid[i], b.ts[i], b.q[i], what))
    b.fields[i][field] = b"x"
    b.fields[i][field] = b"x" * (1 + target - one())
    assert one() == target


@pytest.mark.gpu
def test_e109_edges(codec):
    tab, _ = P.hand_table()
    rows = [19, 19, 19, 19, 19, 0, 19]  # row 19 of the table is valid, row 0 has no id
    pick = lambda a: [a[r] for r in rows]
    b = P.Batch([list(tab.fields[r]) for r in rows], tab.cid[rows], tab.ts[rows], tab.q[rows], pick(tab.order_type),
                pick(tab.tif), tab.limit_price[rows], tab.stop_price[rows], tab.present[rows])
    _grow_to(b, 0, P.F_QUOTE, 0, 65534)   # payload text at the limit: encodes
    _grow_to(b, 1, P.F_QUOTE, 0, 65535)   # E109_PAYLOAD
    _grow_to(b, 2, P.F_ID, 1, 65534)      # headers text at the limit: encodes
    _grow_to(b, 3, P.F_ID, 1, 65535)      # E109_HEADERS
    b.fields[4][P.F_MSGID] = b"m" * 65535  # E109_UUID, reported before the headers text it also overflows
    b.fields[5][P.F_MSGID] = b"m" * 65535  # invalid (no id) and E109: validation wins
    for flags, session in ((0, False), (1, True)):
        exp = P.expected(b, TOPIC, None, 1, flags, session, 8, 9)
        assert exp[2].tolist() == [0, P.E109_PAYLOAD, 0, P.E109_HEADERS, P.E109_UUID, 16, 0]
        P.assert_records(P.run_device(codec, b, TOPIC, None, 1, flags, session, 8, 9), exp)
    topic = b"t" * 65535  # every record E109_TOPIC, but for the invalid one
    exp = P.expected(b, topic, None, 1, 1, True, 8, 9)
    assert exp[2].tolist() == [1, 1, 1, 1, 1, 16, 1] and int(exp[1][-1]) == 0
    P.assert_records(P.run_device(codec, b, topic, None, 1, 1, True, 8, 9), exp)


@pytest.mark.gpu
def test_arenas_at_allocation_end(codec):
    """The order arena and the checks arena each end exactly at the end of a 2 MiB allocation, at
    an address that is not 16-byte aligned (as test_gpu_arena_at_allocation_end)."""
    import torch
    b = P.mixed_batch(3000, 77)
    arena, str_len = T.pack_order_fields(b.fields)
    if arena.size % 16 == 0:
        b.fields[0][0] += b"x"
        arena, str_len = T.pack_order_fields(b.fields)
    c_arena, c_len = P.pack2(b.order_type, b.tif)
    if c_arena.size % 16 == 0:  # keep the end unaligned
        b.tif[-1] = b.tif[-1] + b"Z"
        c_arena, c_len = P.pack2(b.order_type, b.tif)
    exp = P.expected(b, TOPIC, None, 77, 1, True, 1, 2)

    def at_end(a):
        buf = torch.zeros(1 << 21, dtype=torch.uint8, device="cuda")
        assert a.size < buf.numel() and (buf.data_ptr() + buf.numel()) % (1 << 21) == 0
        t = buf[buf.numel() - a.size:]
        t.copy_(torch.from_numpy(a.copy()))
        assert t.data_ptr() % 16 or a.size % 16 == 0
        return t

    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
    checks = (at_end(c_arena), dev(c_len, np.int32), dev(b.limit_price, np.float64), dev(b.stop_price, np.float64),
              dev(b.present, np.uint8))
    r = codec.publish_orders_batch(at_end(arena), dev(str_len, np.int32), dev(b.cid, np.int64), dev(b.ts, np.int64),
                                   dev(b.q, np.float64), dev(np.frombuffer(TOPIC, np.uint8), np.uint8), checks=checks,
                                   ts_default=77, leadership_term_id=1, cluster_session_id=2)
    torch.cuda.synchronize()
    got = (r.out.cpu().numpy(), r.out_off.cpu().numpy().view(np.uint64), r.status.cpu().numpy()[:b.n],
           r.error_mask.cpu().numpy().view(np.uint16)[:b.n])
    P.assert_records(got, exp)


@pytest.mark.gpu
def test_empty_batch(codec):
    import torch
    z = lambda dt: torch.zeros(0, dtype=dt, device="cuda")
    one = torch.zeros(1, dtype=torch.uint8, device="cuda")
    off = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    r = codec.publish_orders_batch(one, z(torch.int32), z(torch.int64), z(torch.int64), z(torch.float64),
                                   torch.from_numpy(np.frombuffer(TOPIC, np.uint8).copy()).cuda(), out_off=off,
                                   checks=(one, z(torch.int32), z(torch.float64), z(torch.float64), z(torch.uint8)))
    torch.cuda.synchronize()
    assert int(r.out_off[0]) == 0 and int(off[0]) == 0


@pytest.mark.gpu
def test_side_stream_self_sizing(codec):
    """A self-sized call on a side stream; the default bound is short (700-byte control fields), so
    the regrow reads out_off[n] after that stream."""
    import torch
    b = P.mixed_batch(2000, 11)
    for f in b.fields:
        f[P.F_UUID] = b"\x01" * 700
    exp = P.expected(b, TOPIC, None, 3, 1, True, 1, 2)
    assert int(exp[1][-1]) > 2000 * (1024 + len(TOPIC)) + 64
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = P.run_device(codec, b, TOPIC, None, 3, 1, True, 1, 2, stream=side)
    P.assert_records(got, exp)


@pytest.mark.gpu
def test_side_stream_without_regrow(codec):
    """The asynchronous form (out given, nothing regrown, no synchronisation inside the call) on a
    side stream while torch's current stream is busy: every output, the error masks of the invalid
    orders included, is written by the call's own launches on its own stream, so nothing queued
    on the current stream may touch it afterwards."""
    import torch
    b, txt = mixed(4099)
    exp = P.expected(b, TOPIC, None, 3, 1, True, 1, 2, txt=txt)
    assert (exp[3] != 0).sum() > 1000 and (exp[2] == 0).sum() > 100
    out = torch.empty(int(exp[1][-1]) + 64, dtype=torch.uint8, device="cuda")
    busy = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()

    def occupy():  # work on the current stream that is still running when the side stream's call has ended
        for k in range(16):
            busy.fill_(k)

    got = P.run_device(codec, b, TOPIC, None, 3, 1, True, 1, 2, stream=side, out=out, before_call=occupy)
    P.assert_records(got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("session", [False, True])
def test_round_trip_decode(codec, session):
    """Wire-mode output through sbe_decode_batch(PARSE_MESSAGE): SBE_ST_TM, SBE_FL_WRAPPED when
    framed, and the payload / headers views are the oracle texts."""
    import torch
    n = 2000
    b, ((pay, po), (hdr, ho)) = mixed(4099)
    b = P.Batch(b.fields[:n], b.cid[:n], b.ts[:n], b.q[:n], b.order_type[:n], b.tif[:n], b.limit_price[:n],
                b.stop_price[:n], b.present[:n])
    mask = b.masks()
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
    arena, str_len = T.pack_order_fields(b.fields)
    c_arena, c_len = P.pack2(b.order_type, b.tif)
    r = codec.publish_orders_batch(dev(arena, np.uint8), dev(str_len, np.int32), dev(b.cid, np.int64),
                                   dev(b.ts, np.int64), dev(b.q, np.float64),
                                   dev(np.frombuffer(TOPIC, np.uint8), np.uint8),
                                   checks=(dev(c_arena, np.uint8), dev(c_len, np.int32), dev(b.limit_price, np.float64),
                                           dev(b.stop_price, np.float64), dev(b.present, np.uint8)),
                                   ts_default=11, flags=0, session=session, leadership_term_id=1, cluster_session_id=2)
    dec = codec.decode_batch(r.out, r.out_off, codec.DEC_PARSE_MESSAGE)
    torch.cuda.synchronize()
    d = dec.numpy()
    data, ro, st = r.out.cpu().numpy(), r.out_off.cpu().numpy(), r.status.cpu().numpy()
    valid = np.nonzero(mask == 0)[0]
    assert valid.size > 100 and (st[valid] == 0).all()
    for i in valid:
        rec = data[int(ro[i]):int(ro[i + 1])].tobytes()
        vo, vl = d["view_off"][i], d["view_len"][i]
        assert d["status"][i] == codec.ST_TM
        assert bool(d["flags"][i] & codec.FL_WRAPPED) == session
        assert rec[vo[0]:vo[0] + vl[0]] == TOPIC and rec[vo[2]:vo[2] + vl[2]] == b.fields[i][P.F_MSGID]
        assert rec[vo[3]:vo[3] + vl[3]] == pay[po[i]:po[i + 1]]
        assert rec[vo[4]:vo[4] + vl[4]] == hdr[ho[i]:ho[i + 1]]
