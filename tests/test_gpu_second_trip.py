"""GPU: every size-gated loop on its second trip.

Several kernels hold a loop whose second iteration starts only past a batch size that no other
test (and no benchmark row) reaches: the single-workgroup scans of the block sums carry a running
value from one trip to the next, and the fixed-grid kernels stride over their input.  Each test
here gives a call just enough items for a second, partial trip (tests/bigbatch_lib.py derives the
sizes from the constants of the sources; tests/test_bigbatch_lib.py asserts them) and compares
every documented output with the oracle or restatement the smaller tests of that call use."""
import copy
import functools

import numpy as np
import pytest
import torch

import autocommit_lib as A
import bigbatch_lib as B
import commitfallback_lib as F
import commitsend_lib as CS
import contract_lib as C
import delivery_lib as D
import inflight_lib as I
import publish_lib as P
import report_lib as R
import sbe_testlib as T
import termappend_lib as TA
import termpoll_lib as TP
from test_gpu_report import ANS, FILL32, FILL64, IN, NOT_IN, UNANS, both, filled

pytestmark = pytest.mark.gpu


def dev(a):
    return B.as_tensor(a, "cuda")


def same(got, exp, what):
    """Two arrays (numpy or tensors of one device) are equal; the first differences named if not."""
    if isinstance(got, torch.Tensor):
        assert got.shape == exp.shape, (what, got.shape, exp.shape)
        if torch.equal(got, exp):
            return
        bad = torch.nonzero(got.reshape(-1) != exp.reshape(-1))[:6, 0]
        raise AssertionError(f"{what}: first differences at {bad.tolist()}: got {got.reshape(-1)[bad].tolist()} "
                             f"expected {exp.reshape(-1)[bad].tolist()}")
    msg = C.mismatches(got, exp, 0, what)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------
# reassembly: frag_scan_blocks' carry over chunks of kFsBlk aggregates, frag_copy's stride
# ------------------------------------------------------------------------------------------
def check_reassembly(codec, data, frag_off, flags, shift):
    """sbe_reassemble_fragments with `flags` at `shift` mod 16 against the C oracle: counts,
    msg_off[0..m], every message byte and the carry."""
    exp_out, exp_off, exp_counts = B.oracle_reassemble_arrays(data, frag_off, flags)
    f = C.placed(flags, shift)
    assert f.data_ptr() % 16 == shift
    r = codec.reassemble(dev(data), dev(frag_off), f)
    torch.cuda.synchronize()
    counts = r.counts.cpu().numpy().view(np.uint64)
    same(counts, exp_counts, "counts")
    m = int(counts[0])
    same(r.msg_off[: m + 1].cpu().numpy().view(np.uint64), exp_off, "msg_off")
    same(r.out[: exp_out.size].cpu().numpy(), exp_out, "out")
    return m, int(counts[1])


def test_reassembly_many_messages(codec):
    """Stream (A): more than SBE_FC_MAXB * 4 * kFragGroup messages, so waves of frag_copy take a
    second group of messages, and more than kFsBlk scan blocks."""
    data, frag_off, flags = B.frag_stream_singles()
    m, _ = check_reassembly(codec, data, frag_off, flags, 0)
    c = B.constants()
    assert m >= c["SBE_FC_MAXB"] * 4 * c["kFragGroup"] + 1


@functools.lru_cache(maxsize=None)
def structured_streams():
    return B.frag_streams_structured(C.frag_scan_block())


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name", ["edge", "long", "carry"])
def test_reassembly_across_the_second_trip(codec, name, shift):
    """Streams (B): groups, singles inside them, a stray END, a BEGIN over a BEGIN and the open
    carry across the edge between the first and the second trip of frag_scan_blocks (scan blocks
    kFsBlk - 1 and kFsBlk), with flags at 0 and at 1 mod 16 (frag_singles_before loads 16 aligned
    flag bytes at a time).  One stream cannot hold all of them (a group that spans block kFsBlk
    leaves no room in it for another), so there are three."""
    blk = C.frag_scan_block()
    data, frag_off, flags, k = structured_streams()[name]
    assert flags.size > blk * blk + 2 * blk
    if name == "edge":
        b, e = k["b"], k["e"]
        assert b // blk == blk - 1 and e // blk == blk and B.is_group(flags, b, e) and B.singles_inside(flags, b, e) >= 1
        assert (flags[b + 1:blk * blk] == B.SINGLE).any() and (flags[blk * blk:e] == B.SINGLE).any()
        s = k["stray_end"]  # behind a whole message that follows the group's END: nothing is open
        assert s // blk == blk and flags[s] == B.END and flags[s - 1] == B.SINGLE and flags[s - 2] == B.END
        b1, b2 = k["begin1"], k["begin2"]
        assert b1 // blk == blk and b2 // blk == blk and flags[b1] == B.BEGIN and flags[b2] == B.BEGIN
        assert (flags[b1 + 1:b2] == B.MIDDLE).all() and flags[b2 + 1] == B.END
    elif name == "long":
        b, e = k["b"], k["e"]
        assert b // blk <= blk - 3 and e // blk == blk + 1 and B.is_group(flags, b, e)
        for j in range(b // blk, e // blk + 1):  # singles inside it in every block it touches
            lo, hi = max(b + 1, j * blk), min(e, (j + 1) * blk)
            assert (flags[lo:hi] == B.SINGLE).any(), j
    else:
        b = k["b"]
        assert b // blk < blk and flags[b] == B.BEGIN and np.isin(flags[b + 1:], (B.MIDDLE, B.SINGLE)).all()
    m, carry = check_reassembly(codec, data, frag_off, flags, shift)
    if name == "carry":
        assert carry >= int(frag_off[k["b"] + 1] - frag_off[k["b"]]) and carry > 0


# ------------------------------------------------------------------------------------------
# term poll: the same scan behind tp_frag_scan_blocks, every index shifted by one after a carry
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def poll_block():
    block, payload, frag_off, flags = B.term_poll_block()
    return dev(block), payload, frag_off, flags


@pytest.mark.parametrize("carry_bytes", [0, 1000], ids=["no carry", "carry"])
def test_term_poll_second_trip(codec, carry_bytes):
    """A block of N frames of 32 and 64 bytes, about 50 MB, with a BEGIN / middle / END group
    across fragment kFsBlk * kFsBlk: all six counts, msg_off[0..m], every message byte and the
    carry, against the composition of termpoll_lib (the walk's fragment table is known from how
    the block is built, which test_bigbatch_lib.py holds to the Python walk; the messages are the
    C oracle's).  With a carry the table has an entry in front, so every index moves by one."""
    block, payload, frag_off, flags = poll_block()
    blk = C.frag_scan_block()
    edge = blk * blk
    assert flags.size == B.N and flags[edge - 2: edge + 2].tolist() == [B.BEGIN, B.MIDDLE, B.MIDDLE, B.END]
    carry = TP.carry_bytes(carry_bytes) if carry_bytes else b""
    exp = B.term_poll_expected(int(block.numel()), payload, frag_off, flags, carry)
    bound = carry_bytes + int(block.numel())
    out = torch.full((bound + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    r = codec.term_poll(block, carry=dev(np.frombuffer(carry, np.uint8)) if carry_bytes else None, out=out)
    torch.cuda.synchronize()
    counts = [int(x) for x in r.counts.cpu().numpy().view(np.uint64)]
    assert counts == exp["counts"]
    m = counts[4]
    same(r.msg_off[: m + 1].cpu().numpy().view(np.uint64), exp["msg_off"], "msg_off")
    same(out[: exp["out"].size], dev(exp["out"]), "messages and carry")
    assert exp["out"].size == int(exp["msg_off"][m]) + counts[5] <= bound
    assert bool((out[bound:] == 0xA5).all()), "bytes at or past carry_bytes + block_bytes were written"


# ------------------------------------------------------------------------------------------
# materialize: mat_scan_blocks' carry
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_batch():
    """N tiny decoded records on the device by the pool method: (data, rec_off, dec as the oracle
    describes every record, expected arena, expected arena_off)."""
    data, off, dec = B.small_record_pool()
    pool_arena, pool_arena_off = B.materialize_pool(data, off, dec)
    pick = dev(B.draw(B.N, off.size - 1, 0xB16D))
    d, o = B.assemble(dev(data), dev(off), pick)
    arena, arena_off = B.materialize_expected(dev(pool_arena), dev(pool_arena_off), dev(dec["view_len"]), pick)
    rows = {k: dev(v)[pick].contiguous() for k, v in dec.items()}
    return d, o, rows, arena, arena_off


def decoded(codec, rows):
    return codec.Decoded(*(rows[k] for k in ("status", "flags", "hdr", "ts", "view_off", "view_len")))


def test_materialize_second_trip(codec):
    """More than kMatBlk blocks of kMatBlk records: arena_off[0..5 N] and every arena byte."""
    d, o, rows, arena, arena_off = small_batch()
    total = int(arena_off[-1])
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    m = codec.materialize_views(d, o, decoded(codec, rows), arena=out, arena_capacity=total)
    torch.cuda.synchronize()
    same(m.arena_off, arena_off, "arena_off")
    same(out[:total], arena, "arena")
    assert bool((out[total:] == 0xA5).all())


def test_materialize_capacity_inside_the_second_trip(codec):
    """arena_capacity ends inside block kMatBlk (the first block of the second trip): the offsets
    hold the full layout, the views written are the prefix of the layout that fits, and the arena
    is untouched from the end of the last view written."""
    d, o, rows, arena, arena_off = small_batch()
    blk = B.constants()["kMatBlk"]
    lo, hi = int(arena_off[5 * blk * blk]), int(arena_off[5 * (blk * blk + blk)])
    cap = (lo + hi) // 2 + 3
    assert lo < cap < hi
    out = torch.full((int(arena_off[-1]) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    m = codec.materialize_views(d, o, decoded(codec, rows), arena=out, arena_capacity=cap)
    torch.cuda.synchronize()
    same(m.arena_off, arena_off, "arena_off")
    fits = int(arena_off[arena_off <= cap].max())  # the end of the last view that fits
    assert cap - 8 <= fits <= cap
    same(out[:fits], arena[:fits], "arena")
    assert bool((out[fits:] == 0xA5).all())


# ------------------------------------------------------------------------------------------
# Order JSON and publish_orders: order_json_scan_blocks' carry (4 * kScanThreads values a trip)
# ------------------------------------------------------------------------------------------
TOPIC = b"orders"


@functools.lru_cache(maxsize=None)
def order_pool():
    """Edge and random Orders with their checks (publish_lib.mixed_batch: hard strings, edge and
    random doubles, every validation failure), and the oracle's two JSON texts of each."""
    b = P.mixed_batch(2048, 0xB16E)
    arena, str_len = T.pack_order_fields(b.fields)
    return b, arena, str_len, P.texts(b)


def picked_orders(pk):
    """The Order arrays of the batch `pk` draws from the pool, as order_to_json_batch takes them."""
    b, arena, str_len, _ = order_pool()
    a, _ = pk.ranges(arena, B.rows_offsets(str_len.sum(1)))
    return a, pk.rows(str_len), pk.rows(b.cid), pk.rows(b.ts), pk.rows(b.q)


@pytest.mark.parametrize("what", [0, 1])
def test_order_json_second_trip(codec, what):
    """N Orders: out_off, status and the whole text, payload JSON and publish headers."""
    b, _, _, txt = order_pool()
    pk = B.Picked(dev(B.draw(B.N, b.n, 0xB16F + what)))
    exp, exp_off = pk.ranges(*txt[what])
    total = int(exp_off[-1])
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    r = codec.order_to_json_batch(*picked_orders(pk), what=what, out=out, out_capacity=total)
    torch.cuda.synchronize()
    same(r.out_off, exp_off, "out_off")
    assert not bool(r.status[: B.N].any())
    same(out[:total], exp, "text")
    assert bool((out[total:] == 0xA5).all())


@pytest.mark.parametrize("session", [False, True], ids=["bare", "framed"])
def test_publish_orders_second_trip(codec, session):
    """N Orders through sbe_publish_orders_batch with checks (both arenas packed: the string bases
    are scanned by the same kernel): out_off, status, error masks and the whole record stream."""
    b, _, _, txt = order_pool()
    tm_ts = np.arange(b.n, dtype=np.uint64) % 3 * 1_000_003  # every third record takes ts_default
    recs, off, status, mask = P.expected(b, TOPIC, tm_ts, 424242, 1, session, term=-5, sess=2 ** 40 + 9, txt=txt)
    assert (status == 0).sum() >= b.n // 16 and set(range(16, 28)) <= set(status.tolist())
    pk = B.Picked(dev(B.draw(B.N, b.n, 0xB170 + session)))
    exp, exp_off = pk.ranges(b"".join(recs), off)
    total = int(exp_off[-1])
    c_arena, c_len = P.pack2(b.order_type, b.tif)
    checks = (pk.ranges(c_arena, B.rows_offsets(c_len.sum(1)))[0], pk.rows(c_len), pk.rows(b.limit_price),
              pk.rows(b.stop_price), pk.rows(b.present))
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    r = codec.publish_orders_batch(*picked_orders(pk), dev(np.frombuffer(TOPIC, np.uint8)), checks=checks,
                                   tm_timestamp=pk.rows(tm_ts), ts_default=424242, flags=1, session=session,
                                   leadership_term_id=-5, cluster_session_id=2 ** 40 + 9, out=out, out_capacity=total)
    torch.cuda.synchronize()
    same(r.out_off, exp_off, "out_off")
    same(r.status[: B.N], pk.rows(status), "status")
    same(r.error_mask[: B.N], pk.rows(mask), "error_mask")
    same(out[:total], exp, "records")
    assert bool((out[total:] == 0xA5).all())


# ------------------------------------------------------------------------------------------
# commit emit: the same scan over two arrays as one, 2 * (nblk + 1) values
# ------------------------------------------------------------------------------------------
POISON_I64 = CS.POISON - 2 ** 64


@functools.lru_cache(maxsize=None)
def commit_pool():
    """Committed records of every table entry (with and without a sequence number), skipped
    records and records whose topic leaves them to the host, ids of 1..23 bytes; with the expected
    outputs of both calls per pool record: (data, off, plain, with a fallback, clock position).
    clock position: where the 19 decimals of uuid_ns + i stand in a JSON frame (they alone depend
    on the record's place in the batch), or -1."""
    heads = [b"{}", b'{"topic":"alpha"}', b'{"topic":"beta"}', b'{"topic":""}', b'{"topic":"a\\"b"}',
             b'{"topic":"gamma"}', b'{"topic":"delta"}', b'{"topic":12}', b'{"topic":"orders"}']
    recs = []
    for i in range(720):
        mid = bytes([97 + i % 26]) * (1 + i * 7 % 23)
        pl = CS.PSEQ if i % 3 == 0 else CS.P
        if i % 10 == 9:
            recs.append(T.tm_wire([b"orders", b"SUBSCRIBE", mid, pl, b"{}"], i))
        elif i % 10 == 8:
            recs.append(T.ack_wire(mid, b"orders", b"c", i))
        else:
            recs.append(T.tm_wire([b"orders", b"X", mid, pl, heads[i % len(heads)]], 1_000_000 + i))
    data, off, dec, seq = CS.batch(recs)
    plan = A.ref_classify(data, off, dec, F.TOPICS)
    kw = dict(seq=seq, session=True, term=3, sess=4)
    plain = CS.ref_emit(data, off, dec, plan, F.TOPIC_IDS, F.IDENTS, **kw)
    fb = F.ref_emit(data, off, dec, plan, **kw)
    assert {CS.NONE, CS.EMITTED, CS.HOST} == set(plain["status"].tolist())
    assert {F.NONE, F.EMITTED, F.HOST, F.EMITTED_JSON} == set(fb["status"].tolist())
    pos = np.full(len(recs), -1, np.int64)
    for i in np.nonzero(fb["status"] == F.EMITTED_JSON)[0]:
        frame = fb["out"][int(fb["out_off"][i]): int(fb["out_off"][i + 1])].tobytes()
        clock = b"_%d" % (F.UUID0 + int(i))
        assert len(clock) == 20 and frame.count(clock) == 1
        pos[i] = frame.index(clock) + 1
    return data, off, plain, fb, pos


@pytest.mark.parametrize("fallback", [False, True], ids=["plain", "fallback"])
@pytest.mark.parametrize("n", [B.N_COMMIT, B.N])
def test_commit_emit_second_trip(codec, n, fallback):
    """sbe_emit_commit_offsets and _ex with a fallback over n records decoded and classified on the
    device: frames, out_off, status, the compacted index list and the totals."""
    data, off, plain, fb, pos = commit_pool()
    exp1 = fb if fallback else plain
    pk = B.Picked(dev(B.draw(n, off.size - 1, 0xB171 + n)))
    d, ro = pk.ranges(data, off)
    seq = torch.full((n,), POISON_I64, dtype=torch.int64, device="cuda")
    gdec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE, seq=seq)
    ttab = codec.commit_topic_table(F.TOPICS, "cuda")
    gplan = codec.classify_commits(d, ro, gdec, ttab)
    exp, exp_off = pk.ranges(exp1["out"], exp1["out_off"])
    status = pk.rows(exp1["status"])
    if fallback:  # the uuid of a JSON frame ends in the decimals of uuid_ns + i
        at = pk.rows(pos)
        rows = torch.nonzero(at >= 0)[:, 0]
        digits = dev(T._digits(np.uint64(F.UUID0) + rows.cpu().numpy().astype(np.uint64), 19))
        where = (exp_off[rows] + at[rows])[:, None] + torch.arange(19, device="cuda")
        exp[where.reshape(-1)] = digits.reshape(-1)
    total = int(exp_off[-1])
    out = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    r = codec.emit_commit_offsets(d, ro, gdec, gplan, dev(np.asarray(F.TOPIC_IDS, np.uint32)),
                                  codec.commit_identifier_table(F.IDENTS, "cuda"), session=True, leadership_term_id=3,
                                  cluster_session_id=4, out=out, out_capacity=total,
                                  fallback=codec.CommitFallback(ttab, dev(np.frombuffer(F.DEFAULT_IDENT, np.uint8)),
                                                                F.NOW, F.UUID0) if fallback else None)
    torch.cuda.synchronize()
    same(r.out_off, exp_off, "out_off")
    same(r.status, status, "status")
    framed = torch.nonzero((status == CS.EMITTED) | (status == F.EMITTED_JSON))[:, 0]
    totals = r.totals.cpu().numpy().view(np.uint64)
    assert totals.tolist() == [framed.numel(), total, int((status == CS.HOST).sum())]
    same(r.emit_idx[: framed.numel()], framed, "emit_idx")
    same(out[:total], exp, "frames")
    assert bool((out[total:] == 0xEE).all())


# ------------------------------------------------------------------------------------------
# term append: ta_scan_blocks' carry and its running minimum (the first record that stops the call)
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def term_append_runs():
    return {r[0]: r[1:] for r in B.term_append_runs(B.constants()["kMatBlk"])}


@pytest.mark.parametrize("name", ["fits", "late", "early and late"])
def test_term_append_second_trip(codec, name):
    """N records of 0..40 bytes: the whole guarded block, the four counts and rec_tail against the
    restatement bigbatch_lib.term_append_np, which test_bigbatch_lib.py holds on these same arrays
    to the host mirror's serial term_append through its stand-alone program.  `late`: the only
    too-long record lies in a plan block of the second trip, so the minimum arrives there; `early
    and late`: one in block 3 as well, which must win."""
    data, rec_off, block_bytes, stop, long_at = term_append_runs()[name]
    blk = B.constants()["kMatBlk"]
    assert all(i // blk >= blk for i in long_at[-1:]) and (len(long_at) < 2 or long_at[0] // blk == 3)
    exp = B.term_append_np(block_bytes, 64, data, rec_off)
    assert exp["stop"] == stop and exp["appended"] == (min(long_at) if long_at else B.N)
    guard = 64
    buf = torch.full((guard + block_bytes + guard,), TA.SENTINEL, dtype=torch.uint8, device="cuda")
    tail = torch.full((B.N + 2,), -1, dtype=torch.int64, device="cuda")
    version, session, stream, term, base = TA.HEADER
    r = codec.term_append(buf[guard: guard + block_bytes], dev(data), dev(rec_off), 64, None, 1408, B.TA_MAX_LEN,
                          codec.TermHeader(session, stream, term, base, version), rec_tail=tail[: B.N])
    torch.cuda.synchronize()
    counts = [int(x) for x in r.counts.cpu().numpy().view(np.uint64)]
    assert counts == [exp["appended"], exp["next"], exp["payload"], exp["stop"]]
    same(tail[: exp["appended"]], dev(exp["rec_tail"]), "rec_tail")
    assert bool((tail[B.N:] == -1).all())
    same(buf[guard: guard + block_bytes], dev(exp["block"]), "block")
    assert bool((buf[:guard] == TA.SENTINEL).all()) and bool((buf[guard + block_bytes:] == TA.SENTINEL).all())


# ------------------------------------------------------------------------------------------
# latency log: the tile stride of lat_sort_hist / lat_sort_scatter, the stride of lat_report_final
# ------------------------------------------------------------------------------------------
def test_latency_report_second_stride(codec):
    """More samples than kDrSortBlocks tiles of kDrBlk * kDrPer hold, appended in one call: the log,
    then order, sorted values, sum, minimum, maximum and the percentiles (random int64 values, half of
    them from 2000 values: many ties, which stay in log order)."""
    n, rng = B.N_LAT, np.random.default_rng(0xB173)
    lats = np.where(rng.random(n) < 0.5, rng.integers(-1000, 1000, n),
                    rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64, endpoint=True))
    value = np.uint64(0) - lats.view(np.uint64)  # now_ns 0, unit_ns 1: lat = -value mod 2^64
    tag_base = 2 ** 64 - 5
    log = codec.LatencyLog(B.LAT_CAPACITY, "cuda")
    log.append(codec.KeyLookups(torch.full((n,), codec.SENT_FIRST, dtype=torch.uint8, device="cuda"), dev(value), None),
               0, 1, tag_base)
    assert log.header() == {"capacity": B.LAT_CAPACITY, "count": n, "dropped": 0}
    lat, tag = log.samples()
    same(lat, lats, "the log's samples")
    same(tag, np.uint64(tag_base) + np.arange(n, dtype=np.uint64), "the log's tags")
    exp = B.report_np(lats)
    assert len(np.unique(exp["sorted"])) < n - 500_000
    before = log.log.clone()
    cap, pct = B.LAT_CAPACITY, R.REPORT_PERCENTILES
    out = codec.LatencyReport(filled(1, torch.int64), filled(3, torch.int64), filled(len(pct) + 1, torch.int64),
                              filled(len(pct) + 1, torch.int64), filled(cap, torch.int64), filled(cap, torch.int32))
    log.report(pct, want_order=True, out=out)
    got = out.numpy()
    assert int(got["count"][0]) == n
    for k in ("stats", "pct_value", "pct_index"):
        same(got[k][: len(exp[k])], exp[k], k)
    same(got["sorted"][:n], exp["sorted"], "sorted")
    same(got["order"][:n], exp["order"], "order")
    assert (got["sorted"][n:].view(np.uint64) == FILL64).all() and (got["order"][n:] == FILL32).all()
    plain = log.report(pct).numpy()  # without the order
    for k in ("stats", "pct_value", "pct_index"):
        same(plain[k], exp[k], k + ", no order")
    assert torch.equal(log.log, before)


# ------------------------------------------------------------------------------------------
# inflight tables: the slot strides of dr_list_scan, inf_rehash_kernel and inf_reset_values_kernel
# ------------------------------------------------------------------------------------------
DEC_KEYS = ("status", "flags", "hdr", "ts", "view_off", "view_len")
M64 = 2 ** 64 - 1


def remember16(tbl, model, keys, ts):
    n = len(keys)
    st = tbl.remember(dev(keys.reshape(-1)), dev(np.arange(n, dtype=np.uint32) * np.uint32(B.KEY_BYTES)),
                      dev(np.full(n, B.KEY_BYTES, np.uint32)), dev(ts))
    same(st.cpu().numpy(), model.remember(B.key_list(keys), ts), "remember: status")


def check_table(tbl, model, what):
    """The header and every live entry (key, value, answered mark) against the model; returns the
    live slots."""
    assert tbl.stats_ex() == model.header(tbl.capacity), what
    assert tbl.stats() == {k: v for k, v in model.header(tbl.capacity).items() if k != "answered"}, what
    words = tbl.table[64:].cpu().numpy().view("<u8").reshape(tbl.capacity, 8)
    slots, keys, values, answered = B.table_entries(words)
    order = np.argsort(keys, kind="stable")
    want = sorted(model.inflight)
    assert keys[order].tolist() == want, f"{what}: the live keys"
    same(values[order], np.array([model.inflight[k] & M64 for k in want], np.uint64), f"{what}: values")
    same(answered[order], np.array([k in model.answered for k in want], bool), f"{what}: answered")
    return slots


LISTS = ((NOT_IN, 64), (IN | ANS, 33), (NOT_IN | UNANS, 10), (0, 64), (ANS, 1))


def check_lists(codec, tbl, m, other, m_other, what, lists=LISTS):
    for flags, limit in lists:
        if flags & (IN | NOT_IN):
            both(codec, tbl, m, other, m_other, flags, limit=limit, what=what)
            both(codec, other, m_other, tbl, m, flags, limit=limit, what=what + ", the other way")
        else:
            both(codec, tbl, m, flags=flags, limit=limit, what=what)
            both(codec, other, m_other, flags=flags, limit=limit, what=what + ", the other table")


def test_inflight_tables_second_sweep(codec):
    """A table of 2^20 slots and one of 2^19: stats, list_keys in both directions, reset_values and
    rehash 2^20 -> 2^19 -> 2^20 against the models, with live entries in the slots that only the
    second sweep of each fixed-grid kernel reaches."""
    keys = B.hex_keys(300_000, 0xB174)
    big, mb = codec.Inflight(B.INF_BIG, "cuda"), D.Table()
    remember16(big, mb, keys, np.arange(1, len(keys) + 1, dtype=np.uint64))
    # a quarter of them matched and erased; ids nobody sent among the acks
    acked = np.concatenate([keys[::4], B.hex_keys(1000, 1, lead=b"n")])
    data, off = B.ack_records(acked, 777)
    exp = T.oracle_decode(data, off, T.DEC_EGRESS)
    assert (exp["status"] == T.ST_EG_ACK).all()
    got = big.match_acks(dev(data), dev(off), codec.Decoded(*(dev(exp[k]) for k in DEC_KEYS))).numpy()
    for k, e in zip(("code", "base_ns", "counts"), mb.match(I.acks_of(data, off, exp))):
        same(got[k], e, f"match: {k}")
    asked = keys[1::8]  # answered entries
    got = big.lookup_keys(dev(asked.reshape(-1)), dev(np.arange(len(asked), dtype=np.uint64) * np.uint64(B.KEY_BYTES)),
                          dev(np.full(len(asked), B.KEY_BYTES, np.uint32))).numpy()
    for k, e in zip(("code", "value", "totals"), mb.lookup(B.key_list(asked))):
        same(got[k], e, f"lookup: {k}")
    slots = check_table(big, mb, "the large table")
    sweep = B.constants()["kInfRehashBlocks"] * B.constants()["kInfBlk"]
    assert mb.live == 225_000 and (slots >= sweep).sum() > 100_000 and (slots < sweep).sum() > 100_000
    # the other table: live, answered and erased keys of the first, and keys of its own
    small, ms = codec.Inflight(B.INF_SMALL, "cuda", 9), D.Table()
    remember16(small, ms, np.concatenate([keys[1::4], keys[::16], B.hex_keys(20_000, 2, lead=b"o")]),
               np.full(75_000 + 18_750 + 20_000, 5, np.uint64))
    theirs = keys[1::4][::3]  # a third of the shared keys answered there too
    got = small.lookup_keys(dev(theirs.reshape(-1)), dev(np.arange(len(theirs), dtype=np.uint64) * np.uint64(B.KEY_BYTES)),
                            dev(np.full(len(theirs), B.KEY_BYTES, np.uint32))).numpy()
    for k, e in zip(("code", "value", "totals"), ms.lookup(B.key_list(theirs))):
        same(got[k], e, f"lookup in the small table: {k}")
    s_slots = check_table(small, ms, "the small table")
    for m in (mb, ms):  # the models list sorted(dict): sorted once, every later sort is a single pass
        m.inflight = dict(sorted(m.inflight.items()))
    list_sweep = B.constants()["kDrListBlocks"] * B.constants()["kDrBlk"]
    assert (s_slots >= list_sweep).sum() > 30_000
    before = big.table.clone(), small.table.clone()
    check_lists(codec, big, mb, small, ms, "lists")
    both(codec, big, mb, min_value=150_000, limit=64, what="least value")
    assert torch.equal(big.table, before[0]) and torch.equal(small.table, before[1])
    # rehash down (the source's second sweep moves entries) and up again
    half, mh = big.rehash(B.INF_SMALL), copy.deepcopy(mb)
    mh.rehash()
    check_table(half, mh, "rehashed to 2^19")
    check_lists(codec, half, mh, small, ms, "lists after the rehash down", LISTS[:2])
    again = half.rehash(B.INF_BIG, tag_bits=5)
    a_slots = check_table(again, mh, "rehashed to 2^20")
    assert (a_slots >= sweep).sum() > 100_000
    check_lists(codec, again, mh, small, ms, "lists after the rehash up", LISTS[:2])
    assert torch.equal(big.table, before[0])
    # reset_values: every live value of the large table back to 1, nothing else touched
    big.reset_values()
    mb.reset_values()
    assert np.array_equal(check_table(big, mb, "after reset_values"), slots)
    both(codec, big, mb, min_value=2, limit=64, what="no value above 1")
    both(codec, big, mb, small, ms, NOT_IN, min_value=1, limit=64, what="every value is 1")
