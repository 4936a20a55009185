"""GPU: ack correlation (sbe_inflight_*, codec.Inflight) against the sequential model of
tests/inflight_lib.py, a dict.  Every comparison is exact.  Acks are wire records decoded in
on-egress mode; the descriptors handed to the match call are the oracle's unless a test says
otherwise.  tag_bits 1 sends every probe of an occupied slot with the same tag bit to the
comparison of the key bytes; 0 is the default of 30 bits."""
import numpy as np
import pytest
import torch

import contract_lib as C
import inflight_lib as I
import sbe_testlib as T
from test_gpu_contract import DEC_KEYS, dec_inputs, dev, on_side_stream, u
from test_inflight_lib import SEED

pytestmark = pytest.mark.gpu

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
TAGS = [1, 0]
TS0 = 1_760_000_000_000


def remember(tbl, keys, ts=None, ts_default=0, mask=None):
    arena, off, ln = I.pack_keys(keys)
    st = tbl.remember(dev(arena), dev(off), dev(ln), None if ts is None else dev(np.asarray(ts, np.uint64)),
                      ts_default, None if mask is None else dev(np.asarray(mask, np.uint8)))
    return st.cpu().numpy()


def decoded(codec, recs):
    """(device data, device rec_off, device descriptors of the oracle, the model's acks)."""
    data, off = T.pack_records(recs)
    exp = T.oracle_decode(data, off, T.DEC_EGRESS)
    dec = codec.Decoded(*(dev(exp[k]) for k in DEC_KEYS))
    return dev(data), dev(off), dec, I.acks_of(data, off, exp)


def match(codec, tbl, recs):
    d_in, r_in, dec, acks = decoded(codec, recs)
    return tbl.match_acks(d_in, r_in, dec).numpy(), acks


def same(got, exp, what):
    msg = C.mismatches(np.asarray(got), np.asarray(exp), 0, what)
    assert msg is None, msg


def check_match(got, exp, what="match"):
    for k, e in zip(("code", "base_ns", "counts"), exp):
        same(got[k], e, f"{what}: {k}")


def check_header(tbl, model, capacity):
    assert tbl.stats() == {"capacity": capacity, "live": model.live, "used": model.used}


def acks_for(ids, ts0=TS0):
    return [I.full_ack(k, b"orders", b"c%d" % j, ts0 + j) for j, k in enumerate(ids)]


# ------------------------------------------------------------------------------------------
# the model's hand cases
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag_bits", TAGS)
def test_hand_table(codec, tag_bits):
    tbl, m = codec.Inflight(64, "cuda", tag_bits), I.Model()
    # a duplicate remember keeps the first ts, inside a call and against a live entry
    ts = np.array([10, 20, 30], np.uint64)
    same(remember(tbl, [b"k1", b"k2", b"k1"], ts), m.remember([b"k1", b"k2", b"k1"], ts), "status")
    same(remember(tbl, [b"k2"], [99]), m.remember([b"k2"], [99]), "status")
    check_header(tbl, m, 64)
    # the second ack of one id is unmatched; simple acks and empty ids never match; a
    # TopicMessage and an undecodable record fire no ack callback
    same(remember(tbl, [b""], [5]), m.remember([b""], [5]), "status")  # emplace("") succeeds
    recs = [I.full_ack(b"k1", b"orders", b"c", 500), I.full_ack(b"k1", b"orders", b"c", 600), T.simple_ack(700),
            I.full_ack(b"", b"orders", b"c", 800), I.full_ack(b"nobody", b"orders", b"c", 900),
            T.tm_wire([b"orders", b"X", b"k2", b"{}", b"{}"], 1000) + b"\0" * 8, b"\x01\x02\x03"]
    got, acks = match(codec, tbl, recs)
    assert [a[0] for a in acks] == [T.ST_EG_ACK] * 2 + [T.ST_EG_ACK_SIMPLE] + [T.ST_EG_ACK] * 2 + [T.ST_EG_TM, T.ST_EG_NONE]
    exp = m.match(acks)
    assert list(exp[0]) == [I.ACK_MATCHED, I.ACK_UNMATCHED, I.ACK_UNMATCHED, I.ACK_UNMATCHED, I.ACK_UNMATCHED,
                            I.ACK_NONE, I.ACK_NONE]
    assert int(exp[1][0]) == 10 and list(exp[2]) == [1, 4]
    check_match(got, exp)
    check_header(tbl, m, 64)
    # remember after a match re-inserts, with the new ts
    same(remember(tbl, [b"k1", b"k2"], [0, 7], ts_default=77), m.remember([b"k1", b"k2"], [0, 7], 77), "status")
    got, acks = match(codec, tbl, acks_for([b"k2", b"k1"]))
    exp = m.match(acks)
    assert list(exp[0]) == [I.ACK_MATCHED] * 2 and list(exp[1]) == [20, 77]
    check_match(got, exp)
    check_header(tbl, m, 64)
    assert (m.live, m.used) == (1, 4)  # "" is still there; the erased slot of k1 was not reused


@pytest.mark.parametrize("tag_bits", TAGS)
def test_empty_batches(codec, tag_bits):
    tbl = codec.Inflight(64, "cuda", tag_bits)
    assert remember(tbl, []).size == 0
    got, _ = match(codec, tbl, [])
    assert got["code"].size == 0 and list(got["counts"]) == [0, 0]
    assert tbl.stats() == {"capacity": 64, "live": 0, "used": 0}


# ------------------------------------------------------------------------------------------
# sizes: partial and several workgroups; small tables force long chains that wrap at the end
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag_bits", TAGS)
@pytest.mark.parametrize("capacity", [64, 128, 1024])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes(codec, n, capacity, tag_bits):
    rng = np.random.default_rng(1000 * n + capacity)
    distinct = min(n, capacity - 8)  # used + distinct new keys < capacity: no record is FULL
    pool = [k for k in I.key_pool(distinct + 12, n) if len(k) <= I.KEY_MAX][:distinct]
    keys = [pool[i] for i in rng.integers(0, len(pool), n)]
    ts = rng.integers(1, 2 ** 63, n, dtype=np.uint64)
    tbl, m = codec.Inflight(capacity, "cuda", tag_bits), I.Model()
    same(remember(tbl, keys, ts), m.remember(keys, ts), "status")
    check_header(tbl, m, capacity)
    ids = [pool[i] if i < len(pool) else b"stranger%d" % i for i in rng.integers(0, len(pool) + 5, n)]
    got, acks = match(codec, tbl, acks_for(ids))
    assert len(acks) == n
    check_match(got, m.match(acks))
    check_header(tbl, m, capacity)
    if n == 257 and capacity == 64:
        assert m.used >= 50  # the chains of a table this full are long and wrap around its end


# ------------------------------------------------------------------------------------------
# random sequences of calls on one table
# ------------------------------------------------------------------------------------------
def run_ops(codec, tbl, ops, model=None):
    """Every call's outputs and header counters; compared with the model after each call when given."""
    outs = []
    for c, op in enumerate(ops):
        if op[0] == "remember":
            got = remember(tbl, op[1], op[2], 5, op[3])
            if model:
                same(got, model.remember(op[1], op[2], 5, op[3]), f"call {c}: status")
            outs.append(got)
        else:
            got, acks = match(codec, tbl, op[1])
            if model:
                check_match(got, model.match(acks), f"call {c}")
            outs.extend(got[k] for k in ("code", "base_ns", "counts"))
        st = tbl.stats()
        if model:
            assert st == {"capacity": tbl.capacity, "live": model.live, "used": model.used}, c
        outs.append(np.array([st["live"], st["used"]]))
    return outs


def test_random_sequence(codec):
    pool, ops = I.random_ops(SEED)  # tests/test_inflight_lib.py checks what this sequence holds
    runs = []
    for tag_bits in TAGS:
        m = I.Model()
        runs.append(run_ops(codec, codec.Inflight(2048, "cuda", tag_bits), ops, m))
        assert all(v >= 20 for v in m.seen.values()), m.seen
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------
# keys, ts, mask, stride
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag_bits", TAGS)
def test_keys_that_differ_in_one_place_are_distinct(codec, tag_bits):
    keys = [b"a", b"a\0", b"a\0\0", b"b", b"", b"\0", b"x" * 39 + b"y", b"x" * 40, b"x" * 39, b"x" * 38 + b"\0",
            b"pub_1760000000000000000", b"pub_1760000000000000001", b"pub_176000000000000000"]
    ts = np.arange(1, len(keys) + 1, dtype=np.uint64)
    tbl, m = codec.Inflight(64, "cuda", tag_bits), I.Model()
    got = remember(tbl, keys, ts)
    assert list(got) == [I.INF_INSERTED] * len(keys)
    same(got, m.remember(keys, ts), "status")
    got, acks = match(codec, tbl, acks_for(list(reversed(keys)) + [b"a\0\0\0", b"x" * 38, b"pub_17600000000000000"]))
    exp = m.match(acks)
    assert list(exp[0]) == [I.ACK_MATCHED if k else I.ACK_UNMATCHED for k in reversed(keys)] + [I.ACK_UNMATCHED] * 3
    check_match(got, exp)
    check_header(tbl, m, 64)


@pytest.mark.parametrize("tag_bits", TAGS)
def test_mask_and_ts_rules(codec, tag_bits):
    tbl, m = codec.Inflight(64, "cuda", tag_bits), I.Model()
    keys = [b"a", b"b", b"z" * 41, b"c", b"d", b"a"]
    ts, mask = np.array([0, 5, 6, 7, 0, 8], np.uint64), np.array([1, 0, 1, 1, 1, 0], np.uint8)
    exp = m.remember(keys, ts, 42, mask)
    assert list(exp) == [I.INF_INSERTED, I.INF_SKIPPED, I.INF_KEY_TOO_LONG, I.INF_INSERTED, I.INF_INSERTED, I.INF_SKIPPED]
    same(remember(tbl, keys, ts, 42, mask), exp, "status")
    same(remember(tbl, [b"e", b"b"], None, 9), m.remember([b"e", b"b"], None, 9), "status")  # ts == NULL
    assert m.inflight == {b"a": 42, b"c": 7, b"d": 42, b"e": 9, b"b": 9}
    check_header(tbl, m, 64)
    got, acks = match(codec, tbl, acks_for([b"e", b"d", b"z" * 41, b"c", b"b", b"a"]))
    exp = m.match(acks)
    assert list(exp[0]) == [I.ACK_MATCHED] * 2 + [I.ACK_LONG_ID] + [I.ACK_MATCHED] * 3
    check_match(got, exp)
    check_header(tbl, m, 64)
    # status is optional
    arena, off, ln = I.pack_keys([b"f"])
    rc = codec.lib().sbe_inflight_remember(tbl.table.data_ptr(), dev(arena).data_ptr(), dev(off).data_ptr(),
                                           dev(ln).data_ptr(), 1, None, 3, None, 1, None, tbl._ws.data_ptr(),
                                           tbl._ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    m.remember([b"f"], None, 3)
    check_header(tbl, m, 64)


def tm_columns(n, seed):
    """A 5-field TopicMessage batch with explicit offsets: (arena, str_off [n,5], str_len [n,5], ts, uuids)."""
    rng = np.random.default_rng(seed)
    uuids = [b"pub_%d" % (1_760_000_000_000_000_000 + int(v)) for v in rng.choice(10 ** 6, n, replace=False)]
    fields = [[b"orders", b"CREATE_ORDER", uu, b'{"qty":%d}' % i, b"{}"] for i, uu in enumerate(uuids)]
    L = np.array([[len(f) for f in r] for r in fields], np.uint32)
    flat = np.frombuffer(b"".join(b"".join(r) for r in fields), np.uint8).copy()
    off = (np.cumsum(L.reshape(-1)) - L.reshape(-1)).astype(np.uint32).reshape(n, 5)
    ts = rng.integers(1, 2 ** 62, n, dtype=np.uint64)
    ts[::9] = 0
    return flat, off, L, ts, uuids


@pytest.mark.parametrize("tag_bits", TAGS)
def test_stride_takes_the_uuid_column(codec, tag_bits):
    n = 130
    arena, off, L, ts, uuids = tm_columns(n, 3)
    tbl, m = codec.Inflight(512, "cuda", tag_bits), I.Model()
    st = tbl.remember(dev(arena), dev(off).view(-1)[2:], dev(L).view(-1)[2:], dev(ts), ts_default=11, stride=5)
    assert st.numel() == n
    same(st.cpu().numpy(), m.remember(uuids, ts, 11), "status")
    got, acks = match(codec, tbl, acks_for(uuids[::-1]))
    exp = m.match(acks)
    assert list(exp[0]) == [I.ACK_MATCHED] * n
    check_match(got, exp)


# ------------------------------------------------------------------------------------------
# a full table
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag_bits", TAGS)
def test_full_table(codec, tag_bits):
    keys = [b"pub_%d" % (TS0 + i) for i in range(100)]
    ts = np.arange(1, 101, dtype=np.uint64)
    tbl = codec.Inflight(64, "cuda", tag_bits)
    st = remember(tbl, keys, ts)
    assert set(st) == {I.INF_INSERTED, I.INF_FULL}
    assert int((st == I.INF_INSERTED).sum()) == 64 and int((st == I.INF_FULL).sum()) == 36
    assert tbl.stats() == {"capacity": 64, "live": 64, "used": 64}
    got, acks = match(codec, tbl, acks_for(keys))
    same(got["code"], np.where(st == I.INF_INSERTED, I.ACK_MATCHED, I.ACK_UNMATCHED), "code")
    same(got["base_ns"], np.where(st == I.INF_INSERTED, ts, np.array([a[2] for a in acks], np.uint64)), "base_ns")
    same(got["counts"], [64, 36], "counts")
    assert tbl.stats() == {"capacity": 64, "live": 0, "used": 64}
    # erased slots are not reused: the table stays full until it is rehashed
    assert list(remember(tbl, [b"late"], [5])) == [I.INF_FULL]
    fresh = tbl.rehash(64)
    assert list(remember(fresh, [b"late"], [5])) == [I.INF_INSERTED]


# ------------------------------------------------------------------------------------------
# rehash
# ------------------------------------------------------------------------------------------
def test_rehash_keeps_every_live_entry(codec):
    pool, ops = I.random_ops(SEED)
    src, m = codec.Inflight(2048, "cuda", 1), I.Model()
    run_ops(codec, src, ops[:13], m)  # ends on a remember: the table holds live and erased entries
    live, used = m.live, m.used
    assert 100 < live < 500 and used > live + 100
    before = src.table.clone()
    small, large = src.rehash(512), src.rehash(4096, tag_bits=0)
    torch.cuda.synchronize()
    assert torch.equal(src.table, before)
    for t, cap in ((small, 512), (large, 4096)):
        assert t.stats() == {"capacity": cap, "live": live, "used": live}
    recs = acks_for(pool)
    exp, _ = match(codec, src, recs)
    assert int(exp["counts"][0]) == live - (b"" in m.inflight)
    for t in (small, large):
        got, _ = match(codec, t, recs)
        check_match(got, [exp[k] for k in ("code", "base_ns", "counts")], "copy")
    with pytest.raises(codec.SbeError):
        codec.Inflight(64, "cuda").rehash(96)


# ------------------------------------------------------------------------------------------
# the call contract (tests/contract_lib.py)
# ------------------------------------------------------------------------------------------
class ContractCase:
    """One remember and one match call on a fresh table of 256 slots, with everything the model
    expects of them."""
    CAP = 256

    def __init__(self, codec, n, seed):
        rng = np.random.default_rng(seed)
        pool = I.key_pool(120, seed)
        self.n = n
        self.keys = [pool[i] for i in rng.integers(0, len(pool), n)]
        self.ts = rng.integers(1, 2 ** 63, n, dtype=np.uint64)
        self.ts[::5] = 0
        self.mask = (rng.integers(0, 6, n) != 0).astype(np.uint8)
        arena, off, ln = I.pack_keys(self.keys)
        self.host_in = [arena, off, ln, self.ts, self.mask]
        self.dev_in = [C.placed(arena, 1), C.placed(off, 4), C.placed(ln, 4), C.placed(self.ts, 8), C.placed(self.mask, 1)]
        recs = I.ack_records(rng, [pool[i] for i in rng.integers(0, len(pool), n)], TS0)
        self.data, self.off = T.pack_records(recs)
        self.m = len(recs)
        self.exp_dec = T.oracle_decode(self.data, self.off, T.DEC_EGRESS)
        self.d_in, self.r_in, self.dec = C.placed(self.data, 16), C.placed(self.off, 8), dec_inputs(codec, self.exp_dec)
        model = I.Model()
        self.status = model.remember(self.keys, self.ts, 5, self.mask)
        self.live1, self.used = model.live, model.used
        self.acks = I.acks_of(self.data, self.off, self.exp_dec)
        self.code, self.base, self.counts = model.match(self.acks)
        self.live2 = model.live
        self.ws_bytes = int(codec.lib().sbe_inflight_workspace_size(max(n, self.m)))

    def inputs_unchanged(self):
        for t, h in zip(self.dev_in + [self.d_in, self.r_in], self.host_in + [self.data, self.off]):
            assert np.array_equal(u(t).reshape(-1), np.asarray(h).reshape(-1))


@pytest.mark.parametrize("n", [1, 65, 257])
def test_calls_write_their_outputs_only(codec, n):
    cs = ContractCase(codec, n, 40 + n)
    if n > 1:
        assert len(set(cs.status)) == 4 and len(set(cs.code)) == 4

    def one(run):
        table = run.buf("table", codec.Inflight.table_bytes(cs.CAP), U8, align=64)
        tbl = codec.Inflight(cs.CAP, "cuda", 1, table=table)
        status, ws = run.buf("status", n, U8), run.buf("workspace", cs.ws_bytes, U8, align=4)
        arena, off, ln, ts, mask = cs.dev_in
        tbl.remember(arena, off, ln, ts, 5, mask, status=status, workspace=ws)
        torch.cuda.synchronize()
        run.expect("status", cs.status)
        assert tbl.stats() == {"capacity": cs.CAP, "live": cs.live1, "used": cs.used}
        out = codec.AckMatches(run.buf("code", cs.m, U8), run.buf("base_ns", cs.m, I64), run.buf("counts", 2, I64))
        tbl.match_acks(cs.d_in, cs.r_in, cs.dec, out=out, workspace=run.buf("workspace2", cs.ws_bytes, U8, align=4))
        torch.cuda.synchronize()
        run.expect("code", cs.code)
        run.expect("base_ns", cs.base)
        run.expect("counts", cs.counts)
        assert tbl.stats() == {"capacity": cs.CAP, "live": cs.live2, "used": cs.used}
        cs.inputs_unchanged()
    C.twice(one)


@pytest.mark.parametrize("a,b", [(0, 70), (65, 130), (129, 131)])
def test_match_on_a_slice_of_a_batch(codec, a, b):
    """rec_off + a and the descriptor arrays advanced by `a` records: rows a..b of the larger
    batch's outputs are filled in place, the rows outside keep the poison."""
    cs = ContractCase(codec, 200, 7)
    assert b <= cs.m
    model = I.Model()
    model.remember(cs.keys, cs.ts, 5, cs.mask)
    code, base, counts = model.match(cs.acks[a:b])
    arena, off, ln, ts, mask = cs.dev_in

    def one(run):
        tbl = codec.Inflight(cs.CAP, "cuda", 1)
        tbl.remember(arena, off, ln, ts, 5, mask)
        full = {k: run.buf(k, cs.m, t) for k, t in (("code", U8), ("base_ns", I64))}
        out = codec.AckMatches(full["code"][a:b], full["base_ns"][a:b], run.buf("counts", 2, I64))
        dec = codec.Decoded(*(getattr(cs.dec, k)[a:b] for k in DEC_KEYS))
        tbl.match_acks(cs.d_in, cs.r_in[a: b + 1], dec, out=out, workspace=run.buf("workspace", 4 * (b - a), U8, align=4))
        torch.cuda.synchronize()
        run.expect("code", code, lo=a)
        run.expect("base_ns", base, lo=a)
        run.expect("counts", counts)
        for k, item in (("code", 1), ("base_ns", 8)):
            run.expect_poison(k, 0, a * item)
            run.expect_poison(k, b * item, cs.m * item)
    C.twice(one)


def test_every_launch_runs_on_the_callers_stream(codec):
    """init, remember, match and rehash queued on a side stream while the current stream is busy."""
    cs = ContractCase(codec, 1500, 11)
    cap = 4096
    arena, off, ln, ts, mask = (dev(h) for h in cs.host_in)
    d_in, r_in = dev(cs.data), dev(cs.off)
    dec = codec.Decoded(*(dev(cs.exp_dec[k]) for k in DEC_KEYS))
    size = codec.Inflight.table_bytes(cap)
    bufs = dict(table=torch.empty(size, dtype=U8, device="cuda"), copy=torch.empty(size, dtype=U8, device="cuda"),
                status=torch.empty(cs.n, dtype=U8, device="cuda"), workspace=torch.empty(cs.ws_bytes, dtype=U8, device="cuda"),
                code=torch.empty(cs.m, dtype=U8, device="cuda"), base_ns=torch.empty(cs.m, dtype=I64, device="cuda"),
                counts=torch.empty(2, dtype=I64, device="cuda"), code2=torch.empty(cs.m, dtype=U8, device="cuda"),
                base_ns2=torch.empty(cs.m, dtype=I64, device="cuda"), counts2=torch.empty(2, dtype=I64, device="cuda"))
    assert bufs["table"].data_ptr() % 64 == 0 and bufs["copy"].data_ptr() % 64 == 0

    def call(s):
        tbl = codec.Inflight(cap, "cuda", 1, stream=s, table=bufs["table"])
        tbl.remember(arena, off, ln, ts, 5, mask, stream=s, status=bufs["status"], workspace=bufs["workspace"])
        cp = codec.Inflight(cap, "cuda", 0, stream=s, table=bufs["copy"])
        codec._check(codec.lib().sbe_inflight_rehash(tbl.table.data_ptr(), cp.table.data_ptr(), s.cuda_stream), "rehash")
        tbl.match_acks(d_in, r_in, dec, stream=s, workspace=bufs["workspace"],
                       out=codec.AckMatches(bufs["code"], bufs["base_ns"], bufs["counts"]))
        cp.match_acks(d_in, r_in, dec, stream=s, workspace=bufs["workspace"],
                      out=codec.AckMatches(bufs["code2"], bufs["base_ns2"], bufs["counts2"]))

    def verify(host, poison):
        for name, exp in (("status", cs.status), ("code", cs.code), ("base_ns", cs.base), ("counts", cs.counts),
                          ("code2", cs.code), ("base_ns2", cs.base), ("counts2", cs.counts)):
            msg = C.mismatches(host[name].reshape(-1), np.asarray(exp).reshape(-1), poison, name)
            assert msg is None, msg
        for name, live in (("table", cs.live2), ("copy", cs.live2)):
            assert list(host[name][:24].view("<u8")) == [cap, live, cs.used if name == "table" else cs.live1]

    on_side_stream(bufs, call, verify)


# ------------------------------------------------------------------------------------------
# the product path: publish, remember, decode the acks, match
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag_bits", TAGS)
def test_round_trip_through_publish_and_egress_decode(codec, tag_bits):
    n = 200
    arena, off, L, ts, uuids = tm_columns(n, 17)
    d_arena, d_off, d_len, d_ts = dev(arena), dev(off), dev(L), dev(ts)
    enc = codec.encode_topic_batch(d_arena, d_len, d_ts, str_off=d_off, flags=codec.ENC_PUBLISH_TOPIC, ts_default=123)
    assert int(enc.status.max()) == 0
    eo, eoff, _ = T.oracle_encode(arena, L, ts, off, T.ENC_PUBLISH_TOPIC, 123)
    assert np.array_equal(u(enc.out_off), eoff) and np.array_equal(u(enc.out)[: int(eoff[-1])], eo)
    tbl = codec.Inflight(512, "cuda", tag_bits)
    st = tbl.remember(d_arena, d_off.view(-1)[2:], d_len.view(-1)[2:], d_ts, ts_default=123, stride=5)
    assert st.cpu().numpy().tolist() == [I.INF_INSERTED] * n
    rng = np.random.default_rng(5)
    subset = rng.permutation(n)[:150]
    ids = [uuids[i] for i in subset] + [b"pub_%d" % i for i in range(25)]
    order = rng.permutation(len(ids))
    recs = [I.full_ack(ids[j], b"orders", b"c", TS0 + int(j)) for j in order]
    data, roff = T.pack_records(recs)
    d_in, r_in = dev(data), dev(roff)
    dec = codec.decode_batch(d_in, r_in, mode=codec.DEC_ON_EGRESS)  # the device's own descriptors
    got = tbl.match_acks(d_in, r_in, dec).numpy()
    sent = np.where(ts == 0, np.uint64(123), ts)
    for row, j in enumerate(order):
        if j < 150:
            assert got["code"][row] == I.ACK_MATCHED and got["base_ns"][row] == sent[subset[j]], (row, j)
        else:
            assert got["code"][row] == I.ACK_UNMATCHED, (row, j)
    assert list(got["counts"]) == [150, 25]
    assert tbl.stats() == {"capacity": 512, "live": 50, "used": 200}
