"""GPU: the call contract of every batch entry point of include/sbecodec.h, beyond what the
kernels compute: which arrays a call writes and which bytes it leaves alone, that workspace
contents do not matter, that pointers advanced into a larger batch (sub-ranges, minimal alignment)
work, and that every launch goes to the caller's stream.  Expected values come from the oracle and
the restatements (sbe_testlib, autocommit_lib, publish_lib); every comparison is bit-exact.  The
poison / guard helpers are in contract_lib.py."""
import ctypes
import functools
import math
import time

import numpy as np
import pytest
import torch

import autocommit_lib as A
import contract_lib as C
import publish_lib as P
import sbe_testlib as T
from test_gpu_parity import SHAPES

pytestmark = pytest.mark.gpu

U8, I16, I32, I64 = torch.uint8, torch.int16, torch.int32, torch.int64
TSD = 1_760_000_000_123  # ts_default
TERM, SESS = -5, 2 ** 40 + 9
TOPIC = b"orders"
DEC_KEYS = ("status", "flags", "hdr", "ts", "view_off", "view_len")
DEC_ITEM = {"status": 1, "flags": 1, "hdr": 8, "ts": 8, "view_off": 20, "view_len": 20, "seq": 8}  # bytes a record
ENC_N = [1, 33, 4095, 4097, 8193]   # 32/64-record tiles, 4096/8192-record superblocks
TILE_N = [1, 63, 64, 65, 129]       # 64-record tiles of decode and classify


def dev(a):
    a = np.array(a, order="C")  # a writable copy: torch warns about read-only arrays
    if a.dtype.kind in "ui":
        a = a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(a).cuda()


def u(t):
    """A device tensor as the unsigned numpy array it holds."""
    a = t.cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------
# batches: mixed-length records with E109 and empty records sprinkled in
# ------------------------------------------------------------------------------------------
_TM_EDGES = np.array([[65535, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 65535, 0], [65534, 3, 29, 1, 0],
                      [70000, 1, 1, 1, 1], [0, 0, 0, 0, 70000]], np.uint32)


@functools.lru_cache(maxsize=None)
def tm_batch(n):
    """(arena, str_len [n,5], ts): fields of 0..400 B, every 97th record from 5 on an edge (E109
    fields, an empty record, a 65534-byte field), every 7th timestamp 0."""
    rng = np.random.default_rng(1000 + n)
    L = np.stack([rng.integers(0, 12, n), rng.integers(0, 14, n), rng.integers(0, 30, n), rng.integers(0, 400, n),
                  rng.integers(0, 60, n)], axis=1).astype(np.uint32)
    idx = np.arange(n)[5::97]
    L[idx] = _TM_EDGES[np.arange(idx.size) % len(_TM_EDGES)]
    arena = rng.integers(0, 256, int(L.sum(dtype=np.int64)), dtype=np.uint8)
    ts = rng.integers(1, 2 ** 63, n, dtype=np.uint64)
    ts[::7] = 0
    return arena, L, ts


@functools.lru_cache(maxsize=None)
def lite_batch(n, tmpl):
    arena, L, tid, seq = T.lite_records(n, tmpl)
    L = L.copy()
    idx = np.arange(n)[5::97]
    nf = L.shape[1]
    for j, i in enumerate(idx):
        L[i] = 0
        if j % 3 != 1:  # E109 in field j % nf; every third edge is an empty record
            L[i, j % nf] = 65535 + 100 * (j % 2)
    arena = np.random.default_rng(tmpl + n).integers(0, 256, int(L.sum(dtype=np.int64)), dtype=np.uint8)
    return arena, L, tid, seq


def gather_form(arena, L):
    """The same strings through str_off: the records in reverse order behind 5 lead bytes, with
    0..2 bytes between them (so the arena is neither packed nor aligned)."""
    n, nf = L.shape
    rec_len = L.astype(np.int64).sum(1)
    src = np.concatenate([[0], np.cumsum(rec_len)])[:-1]
    order = np.arange(n)[::-1]
    sizes = rec_len[order] + order % 3
    base = np.empty(n, np.int64)
    base[order] = 5 + np.concatenate([[0], np.cumsum(sizes)])[:-1]
    new = np.full(5 + int(sizes.sum()) + 7, 0xEE, np.uint8)
    for i in range(n):
        new[base[i]: base[i] + rec_len[i]] = arena[src[i]: src[i] + rec_len[i]]
    inner = np.cumsum(L.astype(np.int64), axis=1) - L
    return new, (base[:, None] + inner).astype(np.uint32)


class EncIn:
    """Device inputs of an encode call at their natural alignment and no better."""

    def __init__(self, arena, L, ts, off=None, tid=None):
        self.n = int(L.shape[0])
        self.arena = C.placed(arena if arena.size else np.zeros(16, np.uint8), 1)
        self.L = C.placed(np.asarray(L, np.uint32), 4)
        self.ts = C.placed(np.asarray(ts, np.uint64), 8)
        self.off = None if off is None else C.placed(np.asarray(off, np.uint32), 4)
        self.tid = None if tid is None else C.placed(np.asarray(tid, np.uint32), 4)


def topic_case(n, flags, gather):
    arena, L, ts = tm_batch(n)
    off = None
    if gather:
        arena, off = gather_form(arena, L)
    exp = T.oracle_encode(arena, L, ts, off, flags, TSD)
    ins = EncIn(arena, L, ts, off)
    return ins, exp, lambda codec, **kw: codec.encode_topic_batch(ins.arena, ins.L, ins.ts, str_off=ins.off,
                                                                  flags=flags, ts_default=TSD, **kw)


def session_case(n, flags, gather):
    arena, L, ts = tm_batch(n)
    off = None
    if gather:
        arena, off = gather_form(arena, L)
    exp = T.oracle_encode_session(arena, L, ts, TERM, SESS, off, flags, TSD)
    ins = EncIn(arena, L, ts, off)
    return ins, exp, lambda codec, **kw: codec.encode_session_batch(ins.arena, ins.L, ins.ts, TERM, SESS,
                                                                    str_off=ins.off, flags=flags, ts_default=TSD, **kw)


def lite_case(n, tmpl):
    arena, L, tid, seq = lite_batch(n, tmpl)
    exp = T.oracle_encode_lite(tmpl, arena, L, tid, seq)
    ins = EncIn(arena, L, seq, tid=tid)
    return ins, exp, lambda codec, **kw: codec.encode_lite_batch(tmpl, ins.arena, ins.L, ins.tid, ins.ts, **kw)


def check_encode_contract(codec, ins, exp, call):
    """Part 1 for one encode call: out_off, status and the stream written in both poison runs at
    capacities out_off[n] + 0 / 1 / 7 / 15 with the bytes after the capacity intact; status = NULL;
    a short capacity (overflow records emit no bytes and nothing is written for them)."""
    eo, eoff, est = exp
    n, total = ins.n, int(eoff[-1])
    assert total > 0 and eoff.size == n + 1
    ws_bytes = codec.workspace_size(n)

    def run_at(cap, with_status=True):
        def one(run):
            out = run.buf("out", cap, U8, align=16)
            off = run.buf("out_off", n + 1, I64, align=8)
            st = run.buf("status", n, U8) if with_status else False
            ws = run.buf("workspace", ws_bytes, U8, align=16)
            call(codec, out=out, out_off=off, status=st, workspace=ws)
            torch.cuda.synchronize()
            run.expect("out_off", eoff)
            fits = eoff[1:] <= cap
            over = ~fits & (np.diff(eoff.astype(np.int64)) > 0)
            if with_status:
                run.expect("status", np.where(over, T.ENC_OVERFLOW, est))
            end = int(eoff[1:][fits].max()) if fits.any() else 0  # end of the last record that fits
            run.expect("out", eo[:end])
            if over.any():  # "record does not fit in out_capacity (nothing written)"
                run.expect_poison("out", end, cap)
        C.twice(one)

    for k in (0, 1, 7, 15):  # out_capacity exactly out_off[n], and a little more
        run_at(total + k)
    run_at(total, with_status=False)
    short = int(eoff[2 * n // 3]) + 5
    run_at(short if short < total else total - 1)


@pytest.mark.parametrize("gather", [False, True], ids=["packed", "gather"])
@pytest.mark.parametrize("flags", [0, T.ENC_REF_TRUNCATE8, T.ENC_PUBLISH_TOPIC], ids=["wire", "trunc8", "publish"])
@pytest.mark.parametrize("n", ENC_N)
def test_encode_topic_writes_its_outputs_only(codec, n, flags, gather):
    ins, exp, call = topic_case(n, flags, gather)
    if n >= 33 and flags != T.ENC_PUBLISH_TOPIC:  # E109 records (no bytes) and an empty record (34 B) are present
        assert (exp[2] != 0).any() and (np.diff(exp[1].astype(np.int64)) == 0).any()
    check_encode_contract(codec, ins, exp, call)


@pytest.mark.parametrize("flags,gather", [(T.ENC_REF_TRUNCATE8, False), (0, True)], ids=["trunc8-packed", "wire-gather"])
@pytest.mark.parametrize("n", ENC_N)
def test_encode_session_writes_its_outputs_only(codec, n, flags, gather):
    ins, exp, call = session_case(n, flags, gather)
    check_encode_contract(codec, ins, exp, call)


@pytest.mark.parametrize("tmpl", [301, 201, 202])
@pytest.mark.parametrize("n", ENC_N)
def test_encode_lite_writes_its_outputs_only(codec, n, tmpl):
    ins, exp, call = lite_case(n, tmpl)
    if n >= 33:
        assert (exp[2] != 0).any()
    check_encode_contract(codec, ins, exp, call)


# ------------------------------------------------------------------------------------------
# decoded batches
# ------------------------------------------------------------------------------------------
_SEQ_PAYLOADS = [b'{"_sequence_number":0}', b'{"_sequence_number":17}', b'{"message":{"_sequence_number":"4"}}',
                 b'{"_sequence_number":"x"}', b'{"a":"\\u005fsequence_number"}', b"no json: _sequence_number",
                 b'{"\\u005fsequence_number":123456789012}', b'{"_sequence_number":0.0,"message":{"_sequence_number":9}}',
                 b'{"_sequence_number":18446744073709551615}', b'{"x":"a\\\\b"}']


def _split(out, off):
    raw = out.tobytes()
    return [raw[int(off[i]): int(off[i + 1])] for i in range(off.size - 1)]


@functools.lru_cache(maxsize=None)
def decode_pool():
    """Records of every kind in a fixed shuffled order: every edge record (empty ones included),
    TopicMessages whose payloads carry the sequence key (with value 0 too) or an escape, acks,
    session frames, variable-length orders and Lite records of the three templates."""
    recs = [r for _, r in T.edge_records()]
    for i in range(60):
        tm = T.tm_wire([b"orders", b"T", b"id%d" % i, _SEQ_PAYLOADS[i % len(_SEQ_PAYLOADS)] + b" " * (i % 23), b"{}"], i + 1)
        recs.append(T.session_wrap(tm) if i % 4 == 3 else tm)
    recs += _split(*T.oracle_encode(*T.var_orders(60, seed=31))[:2])
    for tmpl in (301, 201, 202):
        recs += _split(*T.oracle_encode_lite(tmpl, *T.lite_records(30, tmpl))[:2])
    recs += [T.ack_wire(b"msg_%d" % i, b"orders", b"corr%d" % i, 1_760_000_000_000 + i) + b"\0" * (i % 9) for i in range(30)]
    order = np.random.default_rng(5).permutation(len(recs))
    # record 0: flagged, and its sequence number is 0 (the n = 1 batch)
    return [T.tm_wire([b"t", b"T", b"u", _SEQ_PAYLOADS[0], b"{}"], 9)] + [recs[i] for i in order]


@functools.lru_cache(maxsize=None)
def decode_batch_of(n, mode):
    pool = decode_pool()
    recs = (pool * (n // len(pool) + 1))[:n]
    data, off = T.pack_records(recs)
    exp = T.oracle_decode(data, off, mode)
    seq = T.oracle_seq_batch(data, off, exp) if mode == T.DEC_PARSE else None
    return data, off, exp, seq


def flagged(exp):
    return (exp["status"] == T.ST_TM) & ((exp["flags"] & (T.FL_SEQ_KEY | T.FL_SEQ_ESC)) != 0)


def dec_bufs(codec, run, n):
    d = codec.Decoded(run.buf("status", n, U8), run.buf("flags", n, U8), run.buf("hdr", 4 * n, I16, align=8).view(n, 4),
                      run.buf("ts", n, I64), run.buf("view_off", 5 * n, I32).view(n, 5),
                      run.buf("view_len", 5 * n, I32).view(n, 5))
    return d, run.buf("seq", n, I64)


def dec_rows(codec, d, a):
    return codec.Decoded(*(getattr(d, k)[a:] for k in DEC_KEYS))


def dec_inputs(codec, exp):
    """The oracle's descriptors on the device, every array at its minimal alignment."""
    return codec.Decoded(C.placed(exp["status"], 1), C.placed(exp["flags"], 1), C.placed(exp["hdr"], 8),
                         C.placed(exp["ts"], 8), C.placed(exp["view_off"], 4), C.placed(exp["view_len"], 4))


def expect_rows(run, exp, lo, hi, total):
    """Rows lo..hi of the decoded arrays equal exp's rows (exp: the rows only); the others were not written."""
    for k in DEC_KEYS:
        per = exp[k][0].size if exp[k].ndim > 1 else 1
        run.expect(k, exp[k], lo=lo * per)
        run.expect_poison(k, 0, lo * DEC_ITEM[k])
        run.expect_poison(k, hi * DEC_ITEM[k], total * DEC_ITEM[k])


def expect_seq(run, name, exp, exp_seq, lo=0, total=None):
    """seq starts as poison: flagged TopicMessages hold the oracle's value (0 included), every
    other entry still holds the poison."""
    got = run[name].numpy()
    total = got.size if total is None else total
    want = np.full(total, C.poison_value(run.poison, np.uint64), np.uint64)
    if exp_seq is not None:
        f = flagged(exp)
        want[lo: lo + f.size][f] = exp_seq[f]
    msg = C.mismatches(got, want, run.poison, name)
    assert msg is None, msg


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", [T.DEC_PARSE, T.DEC_EGRESS, T.DEC_LITE], ids=["parse", "egress", "lite"])
def test_decode_writes_its_outputs_only(codec, mode, shape):
    for n in TILE_N:
        data, off, exp, exp_seq = decode_batch_of(n, mode)
        if mode == T.DEC_PARSE:
            f = flagged(exp)
            assert f.any() and (exp_seq[f] == 0).any() and (n == 1 or ((exp_seq[f] != 0).any() and (~f).any()))
        d_in, r_in = C.placed(data, 16), C.placed(off, 8)

        def one(run):
            d, seq = dec_bufs(codec, run, n)
            codec.decode_batch(d_in, r_in, mode=mode, out=d, seq=seq, in_bytes=SHAPES[shape](n))
            torch.cuda.synchronize()
            expect_rows(run, exp, 0, n, n)
            expect_seq(run, "seq", exp, exp_seq)  # not parse mode: nothing of seq is written
        C.twice(one)


@pytest.mark.parametrize("n", TILE_N + [4097])  # a thread takes 16 records, a block 4096
def test_eval_sequence_numbers_writes_flagged_entries_only(codec, n):
    data, off, exp, exp_seq = decode_batch_of(n, T.DEC_PARSE)
    d_in, r_in, dec = C.placed(data, 16), C.placed(off, 8), dec_inputs(codec, exp)

    def one(run):
        seq = run.buf("seq", n, I64)
        codec.eval_sequence_numbers(d_in, r_in, dec, seq=seq)
        torch.cuda.synchronize()
        expect_seq(run, "seq", exp, exp_seq)
    C.twice(one)


MAT_N = 1025  # kMatBlk + 1


@pytest.mark.parametrize("mode", [T.DEC_PARSE, T.DEC_LITE], ids=["parse", "lite"])
def test_materialize_writes_its_outputs_only(codec, mode):
    n = MAT_N
    data, off, exp, _ = decode_batch_of(n, mode)
    arena_exp, aoff = T.oracle_materialize(data, off, exp)
    total = int(aoff[-1])
    d_in, r_in, dec = C.placed(data, 16), C.placed(off, 8), dec_inputs(codec, exp)
    ws_bytes = int(codec.lib().sbe_materialize_workspace_size(n))
    ends = aoff[1:].astype(np.int64)

    def run_at(cap):
        def one(run):
            arena = run.buf("arena", cap, U8)
            ao = run.buf("arena_off", 5 * n + 1, I64)
            ws = run.buf("workspace", ws_bytes, U8, align=16)
            codec.materialize_views(d_in, r_in, dec, arena=arena, arena_off=ao, workspace=ws)
            torch.cuda.synchronize()
            run.expect("arena_off", aoff)  # the full layout whatever the capacity
            end = int(ends[ends <= cap].max())
            run.expect("arena", arena_exp[:end])
            run.expect_poison("arena", end, cap)  # past the last view that fits, nothing is written
        C.twice(one)

    run_at(total)
    mid = int(aoff[5 * (n // 2) + 3])
    for cap in (mid + 1, total - 1):  # the capacity cuts a view; the last view alone does not fit
        run_at(cap)


def commit_bufs(codec, run, n, k):
    return codec.CommitPlan(run.buf("cm", n, U8), run.buf("topic_src", n, U8), run.buf("topic_kind", n, U8),
                            run.buf("topic_off", n, I32), run.buf("topic_len", n, I32), run.buf("topic_idx", n, I32),
                            run.buf("last", k, I64), run.buf("count", k + 2, I64))


def expect_commit(run, exp, lo=0, hi=None, total=None):
    for key in A.KEYS:
        run.expect(key, exp[key], lo=0 if key in ("last", "count") else lo)
    if total is not None:
        for key, item in (("cm", 1), ("topic_src", 1), ("topic_kind", 1), ("topic_off", 4), ("topic_len", 4), ("topic_idx", 4)):
            run.expect_poison(key, 0, lo * item)
            run.expect_poison(key, hi * item, total * item)


@pytest.mark.parametrize("n", TILE_N)
def test_classify_commits_writes_its_outputs_only(codec, n):
    recs = A.random_records(n, 300 + n)
    if n == 1:
        recs = [T.tm_wire([b"t", b"X", b"m1", A.P, b'{"topic":"beta"}'], 5)]
    data, off = T.pack_records(recs)
    exp_dec = T.oracle_decode(data, off, T.DEC_PARSE)
    exp = A.ref_classify(data, off, exp_dec, A.TOPICS)
    d_in, r_in, dec = C.placed(data, 16), C.placed(off, 8), dec_inputs(codec, exp_dec)
    table = codec.commit_topic_table(A.TOPICS, "cuda")
    if n >= 63:
        assert int(exp["count"].sum()) >= 5

    def one(run):
        plan = commit_bufs(codec, run, n, len(A.TOPICS))
        codec.classify_commits(d_in, r_in, dec, table, out=plan)
        torch.cuda.synchronize()
        expect_commit(run, exp)
        codec.classify_commits(d_in, r_in, dec, table, out=plan)  # the call initialises last / count itself
        torch.cuda.synchronize()
        expect_commit(run, exp)
    C.twice(one)


def check_reassemble(codec, data_dev, fo_dev, fl_dev, data, frag_off, flags, ws=None):
    """sbe_reassemble_fragments on the device arrays against the oracle on the same host arrays:
    out sized frag_off[n] - frag_off[0] exactly, msg_off [n + 1], counts [2], all guarded."""
    n = int(flags.size)
    msgs, carry = T.oracle_reassemble(data, frag_off, flags)
    e_out, e_off, e_counts = C.reassembled_expected(msgs, carry)
    size = int(frag_off[n] - frag_off[0])
    assert e_out.size <= size
    ws_bytes = int(codec.lib().sbe_reassemble_workspace_size(n))

    def one(run):
        out = run.buf("out", max(size, 1), U8)
        mo = run.buf("msg_off", n + 1, I64)
        counts = run.buf("counts", 2, I64)
        w = ws if ws is not None else run.buf("workspace", ws_bytes, U8, align=16)
        C.reassemble_raw(codec, data_dev, fo_dev, fl_dev, out, mo, counts, w)
        torch.cuda.synchronize()
        run.expect("counts", e_counts)
        run.expect("msg_off", e_off)  # entries 0..m; the header is silent on the others
        run.expect("out", e_out)      # the messages and the carry; silent on the bytes after them
    C.twice(one)
    return len(msgs), len(carry)


def test_reassemble_writes_its_outputs_only(codec):
    n = C.frag_scan_block() + 1  # one scan block plus one fragment
    data, frag_off, flags = T.fragment_stream(n, 77)
    m, _ = check_reassemble(codec, C.placed(data, 1), C.placed(frag_off, 8), C.placed(flags, 1), data, frag_off, flags)
    assert 100 < m < n


@functools.lru_cache(maxsize=None)
def order_case(n, what):
    fields, cid, ts, q = T.order_batch(n, 40 + n, True)
    arena, str_len = T.pack_order_fields(fields)
    exp, exp_off = T.oracle_order_json(arena, str_len, cid, ts, q, what)
    return (arena, str_len, cid, ts, q), np.frombuffer(exp, np.uint8), exp_off


@pytest.mark.parametrize("what", [0, 1], ids=["payload", "headers"])
@pytest.mark.parametrize("n", [1, 257])  # the sizing launches take 256 Orders a block
def test_order_json_writes_its_outputs_only(codec, n, what):
    (arena, str_len, cid, ts, q), exp, exp_off = order_case(n, what)
    ins = (C.placed(arena, 1), C.placed(str_len, 4), dev(cid), dev(ts), dev(q))
    total = int(exp_off[-1])
    ws_bytes = codec.order_json_workspace_size(n)

    def run_at(cap):
        def one(run):
            out = run.buf("out", cap, U8)
            off = run.buf("out_off", n + 1, I64)
            st = run.buf("status", n, U8)
            ws = run.buf("workspace", ws_bytes, U8, align=16)
            codec.order_to_json_batch(*ins, what=what, out=out, out_off=off, status=st, workspace=ws)
            torch.cuda.synchronize()
            run.expect("out_off", exp_off)
            fits = exp_off[1:] <= cap
            run.expect("status", np.where(fits, 0, codec.JSON_OVERFLOW))
            end = int(exp_off[1:][fits].max()) if fits.any() else 0
            run.expect("out", exp[:end])
            if not fits.all():  # "a record past out_capacity is not written"
                run.expect_poison("out", end, cap)
        C.twice(one)

    run_at(total)
    run_at(total + 7)
    run_at(total - 1)


@pytest.mark.parametrize("session", [False, True], ids=["bare", "framed"])
@pytest.mark.parametrize("n", [65, 257])
def test_publish_orders_writes_its_outputs_only(codec, n, session):
    b = P.mixed_batch(n, 500 + n)
    tm_ts = np.arange(n, dtype=np.uint64) % 3 * 1_000_003
    exp = P.expected(b, TOPIC, tm_ts, TSD, 1, session, term=TERM, sess=SESS)
    total = int(exp[1][-1])
    assert (exp[2] == 0).sum() >= 4 and (exp[2] >= 16).sum() >= 4
    ws_bytes = codec.publish_orders_workspace_size(n)

    def run_at(cap):
        def one(run):
            kw = dict(out=run.buf("out", cap, U8, align=16), out_off=run.buf("out_off", n + 1, I64),
                      status=run.buf("status", n, U8), error_mask=run.buf("error_mask", n, I16),
                      workspace=run.buf("workspace", ws_bytes, U8, align=16))
            got = P.run_device(codec, b, TOPIC, tm_ts, TSD, 1, session, term=TERM, sess=SESS, **kw)
            P.assert_records(got, exp, cap=cap)
            run.expect("out_off", exp[1])
            run.expect("error_mask", exp[3])
            fits = exp[1][1:] <= cap
            end = int(exp[1][1:][fits].max())
            run.expect("out", np.frombuffer(b"".join(exp[0]), np.uint8)[:end])
            if not fits.all():
                run.expect_poison("out", end, cap)
        C.twice(one)

    run_at(total)
    run_at(total - 1)


# ------------------------------------------------------------------------------------------
# 2. workspace contents do not matter
# ------------------------------------------------------------------------------------------
def enc_equals(enc, exp, n):
    eo, eoff, est = exp
    msg = C.mismatches(u(enc.out_off)[: n + 1], eoff, 0x5A, "out_off") or \
        C.mismatches(u(enc.status)[:n], est, 0x5A, "status") or \
        C.mismatches(u(enc.out)[: eo.size], eo, 0x5A, "out")
    assert msg is None, msg


def test_encode_workspace_contents_do_not_matter(codec):
    """One workspace, never re-initialised, through five encode calls of different layouts and
    sizes; then the same calls with the workspace filled with 0xFF before each.

    Every workspace word a launch reads is written earlier in the same call:
    encode (topic, session, Lite): sbe_enc_sums writes all kTilesPerSb tile prefixes (tsum) and the
      total (bsum) of every superblock of the call's own carving; the pack kernel reads tsum / bsum
      at clamped indices below those counts; the sink is only ever stored to."""
    steps = [topic_case(8193, 0, False), lite_case(70, 301), session_case(4097, T.ENC_REF_TRUNCATE8, True),
             lite_case(8193, 202), topic_case(33, T.ENC_PUBLISH_TOPIC, False)]
    ws = torch.full((max(codec.workspace_size(s[0].n) for s in steps),), 0x5A, dtype=U8, device="cuda")
    for fill in (None, 0xFF):
        for ins, exp, call in steps:
            if fill is not None:
                ws.fill_(fill)
            out = torch.full((int(exp[1][-1]) + 16,), 0x5A, dtype=U8, device="cuda")
            off = torch.full((ins.n + 1,), 0x5A5A5A5A, dtype=I64, device="cuda")
            st = torch.full((ins.n,), 0x5A, dtype=U8, device="cuda")
            enc = call(codec, out=out, out_off=off, status=st, workspace=ws)
            torch.cuda.synchronize()
            enc_equals(enc, exp, ins.n)


def test_other_workspaces_contents_do_not_matter(codec):
    """Materialize, reassembly, Order JSON and publish: a workspace left by a larger call of the
    same entry point, then filled with 0xFF.

    Every workspace word a launch reads is written earlier in the same call:
    materialize: mat_sums writes tsum of every tile and bsum of every block; mat_scan_blocks scans
      bsum in place; mat_copy reads tsum / bsum at indices clamped below those counts.
    reassemble: frag_reduce writes every block aggregate, frag_scan_blocks scans them in place and
      zeroes big[0]; frag_scan_msgs writes the table entries 0..m and the listed big messages;
      frag_copy reads entries j <= m = counts[0] and big[1..big[0]] only.
    order_to_json: order_json_totals / order_json_measure write blk_str / blk_txt of every block and
      str_base / sz of every Order before the scans and the writing launch read them.
    publish_orders: publish_totals writes blk_str / blk_chk of every block, publish_measure sz, tl,
      str_base of every Order and blk_txt of every block, before the scans and publish_write."""
    big_n, small_n = 3000, 1025

    def both(size_fn, run_one):
        ws = torch.full((int(size_fn(big_n)) + 16,), 0x5A, dtype=U8, device="cuda")
        run_one(big_n, ws)
        run_one(small_n, ws)  # stale from the larger call
        ws.fill_(0xFF)
        run_one(small_n, ws)
        ws.fill_(0xFF)
        run_one(big_n, ws)

    def materialize(n, ws):
        data, off, exp, _ = decode_batch_of(n, T.DEC_PARSE)
        arena_exp, aoff = T.oracle_materialize(data, off, exp)
        arena = torch.full((arena_exp.size + 16,), 0x5A, dtype=U8, device="cuda")
        m = codec.materialize_views(dev(data), dev(off), dec_inputs(codec, exp), arena=arena, workspace=ws)
        torch.cuda.synchronize()
        msg = C.mismatches(u(m.arena_off), aoff, 0x5A, "arena_off") or \
            C.mismatches(u(m.arena)[: arena_exp.size], arena_exp, 0x5A, "arena")
        assert msg is None, msg

    def reassemble(n, ws):
        data, frag_off, flags = T.fragment_stream(n, 70 + n)
        check_reassemble(codec, dev(data), dev(frag_off), dev(flags), data, frag_off, flags, ws=ws)

    def order_json(n, ws):
        (arena, str_len, cid, ts, q), exp, exp_off = order_case(n, 0)
        out = torch.full((exp.size + 16,), 0x5A, dtype=U8, device="cuda")
        r = codec.order_to_json_batch(dev(arena), dev(str_len), dev(cid), dev(ts), dev(q), what=0, out=out, workspace=ws)
        torch.cuda.synchronize()
        msg = C.mismatches(u(r.out_off), exp_off, 0x5A, "out_off") or C.mismatches(u(r.out)[: exp.size], exp, 0x5A, "out")
        assert msg is None and not u(r.status)[:n].any(), msg

    def publish(n, ws):
        b, exp = publish_case(n)
        out = torch.full((int(exp[1][-1]) + 16,), 0x5A, dtype=U8, device="cuda")
        P.assert_records(P.run_device(codec, b, TOPIC, None, TSD, 1, True, TERM, SESS, out=out, workspace=ws), exp)

    both(lambda n: codec.lib().sbe_materialize_workspace_size(n), materialize)
    both(lambda n: codec.lib().sbe_reassemble_workspace_size(n), reassemble)
    both(codec.order_json_workspace_size, order_json)
    both(codec.publish_orders_workspace_size, publish)


@functools.lru_cache(maxsize=None)
def publish_case(n):
    b = P.mixed_batch(n, 900 + n)
    return b, P.expected(b, TOPIC, None, TSD, 1, True, TERM, SESS)


# ------------------------------------------------------------------------------------------
# 3. sub-ranges and minimal alignment
# ------------------------------------------------------------------------------------------
SUB_N = 200


@functools.lru_cache(maxsize=None)
def sub_batch():
    """About 200 records: the classifier's random records and the decode pool's, shuffled."""
    recs = A.random_records(120, 7) + decode_pool()[:80]
    order = np.random.default_rng(9).permutation(len(recs))
    data, off = T.pack_records([recs[i] for i in order])
    exp = T.oracle_decode(data, off, T.DEC_PARSE)
    return data, off, exp, T.oracle_seq_batch(data, off, exp)


@pytest.mark.parametrize("a,b", [(1, 199), (37, 166), (65, 200)])
def test_decode_chain_on_a_slice_of_a_batch(codec, a, b):
    """decode -> eval-seq -> materialize -> classify with every pointer advanced by `a` records:
    rec_off + a (first offset non-zero; 8 mod 16 for odd a), status + a, view_off + 5 a, ...  Rows
    a..b equal the oracle's rows, the rows outside keep the poison."""
    data, off, exp, exp_seq = sub_batch()
    N, n = SUB_N, b - a
    assert off.size == N + 1 and int(off[a]) > 0
    rows = {k: v[a:b] for k, v in exp.items()}
    arena_exp, aoff = T.oracle_materialize(data, off[a: b + 1], rows)
    cm_exp = A.ref_classify(data, off[a: b + 1], rows, A.TOPICS)
    assert flagged(rows).sum() >= 5 and int(cm_exp["count"].sum()) >= 5
    d_in, r_in = dev(data), C.placed(off, 16)  # rec_off + a is 8 mod 16 for odd a
    table = codec.commit_topic_table(A.TOPICS, "cuda")
    mat_ws = torch.full((int(codec.lib().sbe_materialize_workspace_size(n)) + 16,), 0xFF, dtype=U8, device="cuda")

    def one(run):
        full, seq = dec_bufs(codec, run, N)
        dec = codec.decode_batch(d_in, r_in[a: b + 1], mode=codec.DEC_PARSE_MESSAGE, out=dec_rows(codec, full, a),
                                 seq=seq[a:], in_bytes=int(off[b] - off[a]))
        torch.cuda.synchronize()
        expect_rows(run, rows, a, b, N)
        expect_seq(run, "seq", rows, exp_seq[a:b], lo=a, total=N)
        seq2 = run.buf("seq2", N, I64)
        codec.eval_sequence_numbers(d_in, r_in[a: b + 1], dec, seq=seq2[a:])
        arena = run.buf("arena", max(arena_exp.size, 1), U8)
        ao = run.buf("arena_off", 5 * N + 1, I64)
        codec.materialize_views(d_in, r_in[a: b + 1], dec, arena=arena, arena_off=ao[5 * a:], workspace=mat_ws)
        plan = commit_bufs(codec, run, N, len(A.TOPICS))
        sliced = codec.CommitPlan(*(getattr(plan, f)[a:] for f, _ in codec._COMMIT_KEYS[:6]), plan.last, plan.count)
        codec.classify_commits(d_in, r_in[a: b + 1], dec, table, out=sliced)
        torch.cuda.synchronize()
        expect_seq(run, "seq2", rows, exp_seq[a:b], lo=a, total=N)
        run.expect("arena", arena_exp)
        run.expect("arena_off", aoff, lo=5 * a)
        run.expect_poison("arena_off", 0, 40 * a)
        run.expect_poison("arena_off", 8 * (5 * b + 1))
        expect_commit(run, cm_exp, a, b, N)
    C.twice(one)


def check_packed_encode(codec, arena_dev, L_dev, ts_dev, exp, n):
    eo, eoff, est = exp

    def one(run):
        out = run.buf("out", int(eoff[-1]), U8, align=16)
        oo = run.buf("out_off", n + 1, I64, align=8)
        st = run.buf("status", n, U8)
        ws = run.buf("workspace", codec.workspace_size(n), U8, align=16)
        codec.encode_topic_batch(arena_dev, L_dev, ts_dev, ts_default=TSD, out=out, out_off=oo, status=st, workspace=ws)
        torch.cuda.synchronize()
        run.expect("out_off", eoff)
        run.expect("status", est)
        run.expect("out", eo)
    C.twice(one)


@pytest.mark.parametrize("a,b", [(1, 199), (37, 166), (65, 200)])
def test_packed_encode_on_a_slice_of_a_batch(codec, a, b):
    """str_len + 5 a, timestamp + a and the arena advanced by the bytes of records 0..a-1."""
    arena, L, ts = tm_batch(SUB_N)
    starts = np.concatenate([[0], np.cumsum(L.astype(np.int64).sum(1))])
    assert ((L[a:b] > 65534).any(1) | (L[a:b].sum(1) == 0)).any()  # an E109 or an empty record inside the slice
    exp = T.oracle_encode(arena[starts[a]: starts[b]], L[a:b], ts[a:b], None, 0, TSD)
    A_dev, L_dev, t_dev = dev(arena), dev(L), dev(ts)
    check_packed_encode(codec, A_dev[int(starts[a]):], L_dev[a:b], t_dev[a:b], exp, b - a)


@pytest.mark.parametrize("base", list(range(1, 16)))
def test_packed_encode_at_every_arena_base(codec, base):
    arena, L, ts = tm_batch(100)
    exp = T.oracle_encode(arena, L, ts, None, 0, TSD)
    a_dev = C.placed(arena, base)
    assert a_dev.data_ptr() % 16 == base
    check_packed_encode(codec, a_dev, dev(L), dev(ts), exp, 100)


def _slice_starts(flags):
    """(a fragment that begins a message right after one ended, a fragment in the middle of a group)."""
    single = (flags & 0xC0) == 0xC0
    ended = single | ((flags & 0x40) != 0)
    boundary = next(i for i in range(20, flags.size) if ended[i - 1] and (flags[i] & 0x80))
    middle = next(i for i in range(20, flags.size) if flags[i] == 0 and flags[i - 1] in (0x80, 0x00) and
                  not single[i - 1])
    return boundary, middle


@pytest.mark.parametrize("where", ["message_boundary", "inside_group"])
def test_reassemble_a_slice_of_a_fragment_stream(codec, where):
    data, frag_off, flags = T.fragment_stream(300, 123, p_single=0.3)
    boundary, middle = _slice_starts(flags)
    a, b = (boundary if where == "message_boundary" else middle), 293
    assert int(frag_off[a]) > 0
    d_dev, fo_dev, fl_dev = dev(data), C.placed(frag_off, 16), C.placed(flags, 16)
    m, _ = check_reassemble(codec, d_dev, fo_dev[a: b + 1], fl_dev[a:b], data, frag_off[a: b + 1], flags[a:b])
    assert m > 50


def test_pointers_below_their_alignment_are_einval_and_write_nothing(codec):
    """out at 8 mod 16 and out_off at 4 mod 8 (encode), rec_off at 4 mod 8 and seq at 4 mod 8
    (decode, eval-seq): SBE_EINVAL, and no output or workspace byte changes."""
    n, lib = 40, codec.lib()
    arena, L, ts = tm_batch(n)
    eo, eoff, est = T.oracle_encode(arena, L, ts, None, 0, TSD)
    a_dev, L_dev, t_dev = dev(arena), dev(L), dev(ts)
    enc = C.PoisonRun(0xA5)
    out = enc.buf("out", int(eoff[-1]) + 16, U8, align=16)
    oo = enc.buf("out_off", n + 2, I64)
    st = enc.buf("status", n, U8)
    ws = enc.buf("workspace", codec.workspace_size(n), U8, align=16)
    batch = codec._TmBatch(a_dev.data_ptr(), None, L_dev.data_ptr(), t_dev.data_ptr())
    ptr = ctypes.c_void_p

    def encode(out_ptr, off_ptr):
        rc = lib.sbe_encode_topic_batch(ctypes.byref(batch), n, TSD, 0, ptr(out_ptr), int(eoff[-1]), ptr(off_ptr),
                                        ptr(st.data_ptr()), ptr(ws.data_ptr()), ws.numel(), None)
        torch.cuda.synchronize()
        return rc

    m = 65
    data, off, exp, exp_seq = decode_batch_of(m, T.DEC_PARSE)
    d_in, r_in = dev(data), dev(off)
    r_mis = torch.zeros(8 * off.size + 8, dtype=U8, device="cuda")  # the same offsets at 4 mod 8
    r_mis[4: 4 + 8 * off.size] = r_in.view(U8)
    dec = C.PoisonRun(0xA5)
    d, _ = dec_bufs(codec, dec, m)
    seq = dec.buf("seq", m + 1, I64)
    dec_ok = dec_inputs(codec, exp)
    torch.cuda.synchronize()

    def decode(rec_ptr, seq_ptr):
        dd = codec._Decoded(*(getattr(d, k).data_ptr() for k in DEC_KEYS), seq_ptr)
        rc = lib.sbe_decode_batch(ptr(d_in.data_ptr()), ptr(rec_ptr), m, codec.DEC_PARSE_MESSAGE, ctypes.byref(dd), None)
        torch.cuda.synchronize()
        return rc

    def eval_seq(rec_ptr, seq_ptr):
        dd = codec._Decoded(*(getattr(dec_ok, k).data_ptr() for k in DEC_KEYS), None)
        rc = lib.sbe_eval_sequence_numbers(ptr(d_in.data_ptr()), ptr(rec_ptr), m, ctypes.byref(dd), ptr(seq_ptr), None)
        torch.cuda.synchronize()
        return rc

    assert out.data_ptr() % 32 == 16 and oo.data_ptr() % 16 == 8 and seq.data_ptr() % 16 == 8
    assert encode(out.data_ptr() + 8, oo.data_ptr()) == -1
    assert encode(out.data_ptr(), oo.data_ptr() + 4) == -1
    assert decode(r_mis.data_ptr() + 4, seq.data_ptr()) == -1
    assert decode(r_in.data_ptr(), seq.data_ptr() + 4) == -1
    assert eval_seq(r_mis.data_ptr() + 4, seq.data_ptr()) == -1
    assert eval_seq(r_in.data_ptr(), seq.data_ptr() + 4) == -1
    for run in (enc, dec):
        for name in run.bufs:
            run.expect_poison(name)
        run.check_guards()
    # the same calls with aligned pointers are accepted and write
    assert encode(out.data_ptr(), oo.data_ptr()) == 0 and decode(r_in.data_ptr(), seq.data_ptr()) == 0
    enc.expect("out_off", eoff)
    enc.expect("status", est)
    enc.expect("out", eo)
    expect_rows(dec, exp, 0, m, m)
    expect_seq(dec, "seq", exp, exp_seq, total=m + 1)
    enc.check_guards()
    dec.check_guards()


# ------------------------------------------------------------------------------------------
# 4. all work goes to the caller's stream
# ------------------------------------------------------------------------------------------
_SIDE = []


def side_stream(busy):
    """A stream that runs beside torch's current stream.  HIP maps streams onto a few hardware
    queues, and two streams that share one run in order: on such a stream everything waits for the
    busy work and the test could show nothing.  So candidates are probed once: a fill queued on the
    candidate must end while the current stream is still busy."""
    if _SIDE:
        return _SIDE[0]
    probe = torch.empty(64, dtype=U8, device="cuda")
    for _ in range(16):
        cand = torch.cuda.Stream()
        torch.cuda.synchronize()
        for k in range(40):
            busy.fill_(k)
        done = torch.cuda.Event()
        done.record()
        with torch.cuda.stream(cand):
            probe.fill_(1)
        cand.synchronize()
        beside = not done.query()
        torch.cuda.synchronize()
        if beside:
            _SIDE.append(cand)
            return cand
    pytest.fail("no stream runs beside the current stream: the side-stream tests can show nothing")


def on_side_stream(bufs, call, verify):
    """Every output and workspace in `bufs` is preallocated, so call(stream) allocates nothing and
    reads no size back.  The buffers are poisoned and the device synchronised; torch's current
    stream is then kept busy for many times the duration of the call (measured here on an idle
    device), the call is made on a side stream, only that stream is synchronised and the results
    are copied out on it.  A launch or memset issued on any other stream is still queued behind the
    busy work, and its outputs hold the poison.  If the busy work is found finished, the test
    fails: it would have shown nothing."""
    busy = torch.empty(1 << 29, dtype=U8, device="cuda")  # a fill takes far longer than queueing it
    side = side_stream(busy)

    def poison(p):
        for t in bufs.values():
            t.view(U8).fill_(p)
        torch.cuda.synchronize()

    poison(C.POISONS[0])
    call(side)  # loads the code objects
    side.synchronize()
    t_call = 1.0
    for _ in range(3):  # the shortest of three: a host hiccup must not inflate the busy work
        poison(C.POISONS[0])
        t0 = time.perf_counter()
        call(side)
        side.synchronize()
        t_call = min(t_call, time.perf_counter() - t0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    busy.fill_(1)
    e1.record()
    torch.cuda.synchronize()
    unit = max(e0.elapsed_time(e1) * 1e-3, 1e-6)
    reps = max(8, math.ceil(30 * max(t_call, 1e-3) / unit))  # at least 30 calls' worth, and 30 ms
    assert reps * unit < 3.0, (t_call, unit)
    poison(C.POISONS[1])
    for k in range(reps):
        busy.fill_(k & 0xFF)
    done = torch.cuda.Event()
    done.record()
    t0 = time.perf_counter()
    call(side)
    side.synchronize()
    t_beside = time.perf_counter() - t0
    running_after_call = not done.query()
    with torch.cuda.stream(side):
        host = {k: u(t) for k, t in bufs.items()}
    running_after_copy = not done.query()
    torch.cuda.synchronize()
    if not (running_after_call and running_after_copy):
        pytest.fail(f"the busy work on the current stream ({reps} fills of {unit * 1e6:.0f} us) had ended before the "
                    f"side stream's results were read (the call took {t_call * 1e6:.0f} us on an idle device, "
                    f"{t_beside * 1e6:.0f} us beside the busy work): the test shows nothing")
    verify(host, C.POISONS[1])


def _need(host, poison, name, exp, lo=0):
    exp = np.asarray(exp).reshape(-1)
    msg = C.mismatches(host[name].reshape(-1)[lo: lo + exp.size], exp, poison, name)
    assert msg is None, msg


def enc_stream_case(codec, case):
    ins, exp, call = case
    bufs = dict(out=torch.empty(int(exp[1][-1]) + 16, dtype=U8, device="cuda"),
                out_off=torch.empty(ins.n + 1, dtype=I64, device="cuda"), status=torch.empty(ins.n, dtype=U8, device="cuda"),
                workspace=torch.empty(codec.workspace_size(ins.n), dtype=U8, device="cuda"))

    def verify(host, poison):
        _need(host, poison, "out_off", exp[1])
        _need(host, poison, "status", exp[2])
        _need(host, poison, "out", exp[0])

    on_side_stream(bufs, lambda s: call(codec, stream=s, **bufs), verify)


def test_encode_topic_runs_on_the_callers_stream(codec):
    enc_stream_case(codec, topic_case(4097, 0, False))


def test_encode_session_runs_on_the_callers_stream(codec):
    enc_stream_case(codec, session_case(4097, T.ENC_REF_TRUNCATE8, False))


def test_encode_lite_runs_on_the_callers_stream(codec):
    enc_stream_case(codec, lite_case(4097, 201))


def _plain_decoded(codec, n):
    d = codec.alloc_decoded(n, "cuda")
    return d, {k: getattr(d, k) for k in DEC_KEYS}


def _need_rows(host, poison, exp):
    for k in DEC_KEYS:
        _need(host, poison, k, exp[k])


def _need_seq(host, poison, name, exp, exp_seq):
    want = np.full(exp_seq.size, C.poison_value(poison, np.uint64), np.uint64)
    f = flagged(exp)
    want[f] = exp_seq[f]
    _need(host, poison, name, want)


def test_decode_with_seq_runs_on_the_callers_stream(codec):
    n = 4097
    data, off, exp, exp_seq = decode_batch_of(n, T.DEC_PARSE)
    d_in, r_in = dev(data), dev(off)
    d, bufs = _plain_decoded(codec, n)
    bufs["seq"] = torch.empty(n, dtype=I64, device="cuda")

    def verify(host, poison):
        _need_rows(host, poison, exp)
        _need_seq(host, poison, "seq", exp, exp_seq)

    on_side_stream(bufs, lambda s: codec.decode_batch(d_in, r_in, out=d, seq=bufs["seq"], stream=s,
                                                      in_bytes=int(off[-1])), verify)


def test_eval_sequence_numbers_runs_on_the_callers_stream(codec):
    n = 4097
    data, off, exp, exp_seq = decode_batch_of(n, T.DEC_PARSE)
    d_in, r_in, dec = dev(data), dev(off), dec_inputs(codec, exp)
    bufs = dict(seq=torch.empty(n, dtype=I64, device="cuda"))
    on_side_stream(bufs, lambda s: codec.eval_sequence_numbers(d_in, r_in, dec, seq=bufs["seq"], stream=s),
                   lambda host, poison: _need_seq(host, poison, "seq", exp, exp_seq))


def test_materialize_runs_on_the_callers_stream(codec):
    n = 4097
    data, off, exp, _ = decode_batch_of(n, T.DEC_PARSE)
    arena_exp, aoff = T.oracle_materialize(data, off, exp)
    d_in, r_in, dec = dev(data), dev(off), dec_inputs(codec, exp)
    bufs = dict(arena=torch.empty(arena_exp.size + 16, dtype=U8, device="cuda"),
                arena_off=torch.empty(5 * n + 1, dtype=I64, device="cuda"),
                workspace=torch.empty(int(codec.lib().sbe_materialize_workspace_size(n)) + 16, dtype=U8, device="cuda"))

    def verify(host, poison):
        _need(host, poison, "arena_off", aoff)
        _need(host, poison, "arena", arena_exp)

    on_side_stream(bufs, lambda s: codec.materialize_views(d_in, r_in, dec, stream=s, **bufs), verify)


def test_classify_commits_runs_on_the_callers_stream(codec):
    n = 1000
    data, off = T.pack_records(A.random_records(n, 55))
    exp_dec = T.oracle_decode(data, off, T.DEC_PARSE)
    exp = A.ref_classify(data, off, exp_dec, A.TOPICS)
    d_in, r_in, dec = dev(data), dev(off), dec_inputs(codec, exp_dec)
    table = codec.commit_topic_table(A.TOPICS, "cuda")
    k = len(A.TOPICS)
    sizes = dict(cm=(n, U8), topic_src=(n, U8), topic_kind=(n, U8), topic_off=(n, I32), topic_len=(n, I32),
                 topic_idx=(n, I32), last=(k, I64), count=(k + 2, I64))
    bufs = {f: torch.empty(c, dtype=t, device="cuda") for f, (c, t) in sizes.items()}
    plan = codec.CommitPlan(**bufs)

    def verify(host, poison):
        for key in A.KEYS:
            _need(host, poison, key, exp[key])

    on_side_stream(bufs, lambda s: codec.classify_commits(d_in, r_in, dec, table, out=plan, stream=s), verify)


def test_reassemble_runs_on_the_callers_stream(codec):
    n = 4 * C.frag_scan_block() + 1
    data, frag_off, flags = T.fragment_stream(n, 91)
    e_out, e_off, e_counts = C.reassembled_expected(*T.oracle_reassemble(data, frag_off, flags))
    d_in, fo, fl = dev(data), dev(frag_off), dev(flags)
    bufs = dict(out=torch.empty(data.size, dtype=U8, device="cuda"), msg_off=torch.empty(n + 1, dtype=I64, device="cuda"),
                counts=torch.empty(2, dtype=I64, device="cuda"),
                workspace=torch.empty(int(codec.lib().sbe_reassemble_workspace_size(n)) + 16, dtype=U8, device="cuda"))

    def verify(host, poison):
        _need(host, poison, "counts", e_counts)
        _need(host, poison, "msg_off", e_off)
        _need(host, poison, "out", e_out)

    on_side_stream(bufs, lambda s: C.reassemble_raw(codec, d_in, fo, fl, bufs["out"], bufs["msg_off"], bufs["counts"],
                                                    bufs["workspace"], stream=s), verify)
