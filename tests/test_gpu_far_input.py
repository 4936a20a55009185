"""GPU: inputs past 4 GiB.

Every consumer of a decoded batch computes in + rec_off[i] + view_off; an offset of 2^32 or more
reached only the topic encoder and the wide decode kernel so far, in the 16 M-record test, so a
truncation to 32 bits anywhere else would be silent.  One tensor of 2^32 + 64 KiB bytes is
allocated once (not filled), a batch of 129 mixed records is copied into it so that it straddles
byte 2^32 (the base 16-byte aligned, byte 2^32 inside the batch's 20 KB record, half of the
records on each side), and every call that takes `in` and `rec_off` runs on the large tensor with
the shifted offsets.  Its outputs are record-relative, so they are compared with what the oracle
and the restatements give for the same records at offset 0."""
import types

import numpy as np
import pytest
import torch

import autocommit_lib as A
import bigbatch_lib as B
import commitsend_lib as CS
import delivery_lib as D
import inflight_lib as I
import jsonpaths_lib as J
import sbe_testlib as T
import select_lib as S
import termappend_lib as TA

pytestmark = pytest.mark.gpu
DEC_KEYS = ("status", "flags", "hdr", "ts", "view_off", "view_len")
POISON_I64 = CS.POISON - 2 ** 64


def dev(a):
    return B.as_tensor(a, "cuda")


def same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.nonzero((got != exp).reshape(-1))[0]
    assert bad.size == 0, (what, bad[:6], got.reshape(-1)[bad[:6]], exp.reshape(-1)[bad[:6]])


@pytest.fixture(scope="module")
def far(codec):
    recs, ack_ids = B.far_records()
    data, off = T.pack_records(recs)
    base = B.far_base(off)
    big = torch.empty(B.FAR_BYTES, dtype=torch.uint8, device="cuda")
    big[base: base + data.size] = dev(data)
    far_off = off + np.uint64(base)
    n = len(recs)
    assert base % 16 == 0 and big.data_ptr() % 16 == 0 and base + data.size <= B.FAR_BYTES
    assert int(far_off[0]) < 2 ** 32 < int(far_off[n])
    assert int(far_off[B.FAR_BIG]) < 2 ** 32 < int(far_off[B.FAR_BIG + 1])  # byte 2^32 lies inside the 20 KB record
    assert (far_off[1:] < 2 ** 32).sum() == B.FAR_BIG and (far_off[:-1] > 2 ** 32).sum() == n - B.FAR_BIG - 1
    ro = dev(far_off)
    dec = T.oracle_decode(data, off, T.DEC_PARSE)
    seq = torch.full((n,), POISON_I64, dtype=torch.int64, device="cuda")
    gdec = codec.decode_batch(big, ro, mode=codec.DEC_PARSE_MESSAGE, seq=seq)
    torch.cuda.synchronize()
    yield types.SimpleNamespace(big=big, ro=ro, data=data, off=off, n=n, recs=recs, ack_ids=ack_ids, dec=dec, gdec=gdec)
    del big


@pytest.mark.parametrize("sized", [False, True], ids=["plain", "sized"])
@pytest.mark.parametrize("mode", [T.DEC_PARSE, T.DEC_EGRESS, T.DEC_LITE])
def test_decode(codec, far, mode, sized):
    """sbe_decode_batch and _sized (with the records' bytes as the hint) in the three modes; parse
    mode with seq."""
    exp = T.oracle_decode(far.data, far.off, mode)
    assert len(set(exp["status"].tolist())) >= 2
    seq = torch.full((far.n,), POISON_I64, dtype=torch.int64, device="cuda") if mode == T.DEC_PARSE else None
    got = codec.decode_batch(far.big, far.ro, mode=mode, seq=seq, in_bytes=int(far.off[-1] - far.off[0]) if sized else 0)
    torch.cuda.synchronize()
    g = got.numpy()
    for k in DEC_KEYS:
        same(g[k], exp[k], k)
    if seq is not None:
        flagged = (exp["status"] == T.ST_TM) & ((exp["flags"] & (T.FL_SEQ_KEY | T.FL_SEQ_ESC)) != 0)
        want = np.where(flagged, T.oracle_seq_batch(far.data, far.off, exp), np.uint64(CS.POISON))
        assert flagged.sum() >= 10 and flagged[B.FAR_BIG]
        same(got.seq.cpu().numpy().view(np.uint64), want, "seq")


def test_eval_sequence_numbers(codec, far):
    plain = codec.Decoded(*(getattr(far.gdec, k) for k in DEC_KEYS))
    got = codec.eval_sequence_numbers(far.big, far.ro, plain)
    torch.cuda.synchronize()
    same(got.cpu().numpy().view(np.uint64), T.oracle_seq_batch(far.data, far.off, far.dec), "seq")


def test_materialize_views(codec, far):
    exp, exp_off = T.oracle_materialize(far.data, far.off, far.dec)
    out = torch.full((exp.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    m = codec.materialize_views(far.big, far.ro, far.gdec, arena=out, arena_capacity=exp.size)
    torch.cuda.synchronize()
    same(m.arena_off.cpu().numpy().view(np.uint64), exp_off, "arena_off")
    same(out.cpu().numpy(), np.concatenate([exp, np.full(64, 0xA5, np.uint8)]), "arena")
    assert exp.size > 20_000


def test_classify_and_emit_commits(codec, far):
    """sbe_classify_commits, then sbe_emit_commit_offsets on its plan."""
    plan = A.ref_classify(far.data, far.off, far.dec, CS.TOPICS)
    gplan = codec.classify_commits(far.big, far.ro, far.gdec, CS.TOPICS)
    torch.cuda.synchronize()
    got = gplan.numpy()
    for k in A.KEYS:
        same(got[k], plan[k], k)
    assert (plan["cm"] == A.COMMIT).sum() >= 30 and plan["cm"][B.FAR_BIG] == A.COMMIT
    seq = T.oracle_seq_batch(far.data, far.off, far.dec)
    exp = CS.ref_emit(far.data, far.off, far.dec, plan, CS.TOPIC_IDS, CS.IDENTS, seq=seq, session=True, term=3, sess=4)
    assert {CS.NONE, CS.EMITTED, CS.HOST} <= set(exp["status"].tolist())
    total = int(exp["out_off"][-1])
    out = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    r = codec.emit_commit_offsets(far.big, far.ro, far.gdec, gplan, CS.TOPIC_IDS, CS.IDENTS, session=True,
                                  leadership_term_id=3, cluster_session_id=4, out=out, out_capacity=total)
    torch.cuda.synchronize()
    g = r.numpy()
    CS.same(g, exp, "far input")
    assert (g["out"][total:] == 0xEE).all()


def test_json_extract(codec, far):
    exp = J.ref_extract(far.data, far.off, far.dec, J.HAND_PATHS)
    got = codec.extract_json(far.big, far.ro, far.gdec, J.HAND_PATHS)
    torch.cuda.synchronize()
    J.same(got.numpy(), exp, "far input", far.data, far.off)
    assert (exp["doc"] == J.OK).sum() >= 40


def test_order_select(codec, far):
    exp = S.model(far.data, far.off, far.dec)
    got = codec.order_select(far.big, far.ro, far.gdec)
    torch.cuda.synchronize()
    S.same(got.numpy(), exp, "far input", ["record %d" % i for i in range(far.n)])


def test_inflight_match_acks(codec, far):
    """Acks on both sides of byte 2^32 against a table that holds two thirds of their ids."""
    exp = T.oracle_decode(far.data, far.off, T.DEC_EGRESS)
    is_ack = np.nonzero(exp["status"] == T.ST_EG_ACK)[0]
    assert (is_ack < B.FAR_BIG).sum() >= 5 and (is_ack > B.FAR_BIG).sum() >= 5
    tbl, m = codec.Inflight(256, "cuda"), D.Table()
    known = [k for i, k in enumerate(far.ack_ids) if i % 3]
    arena, koff, klen = I.pack_keys(known)
    ts = np.arange(100, 100 + len(known), dtype=np.uint64)
    st = tbl.remember(dev(arena), dev(koff), dev(klen), dev(ts))
    same(st.cpu().numpy(), m.remember(known, ts), "remember")
    gdec = codec.decode_batch(far.big, far.ro, mode=codec.DEC_ON_EGRESS)
    got = tbl.match_acks(far.big, far.ro, gdec).numpy()
    want = m.match(I.acks_of(far.data, far.off, exp))
    for k, e in zip(("code", "base_ns", "counts"), want):
        same(got[k], e, k)
    assert int(want[2][0]) == len(known) and int(want[2][1]) == len(far.ack_ids) - len(known)
    assert tbl.stats() == {"capacity": 256, "live": 0, "used": len(known)}


def test_reassemble_fragments(codec, far):
    """The records as fragments: frag_off straddles 2^32."""
    rng = np.random.default_rng(5)
    flags = rng.choice(np.array([B.SINGLE, B.BEGIN, B.END, B.MIDDLE], np.uint8), far.n, p=[0.4, 0.2, 0.2, 0.2])
    flags[B.FAR_BIG - 1: B.FAR_BIG + 2] = (B.BEGIN, B.MIDDLE, B.END)  # the 20 KB fragment inside a group
    exp_out, exp_off, exp_counts = B.oracle_reassemble_arrays(far.data, far.off, flags)
    out = torch.full((far.data.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    r = codec.reassemble(far.big, far.ro, dev(flags), out=out)
    torch.cuda.synchronize()
    same(r.counts.cpu().numpy().view(np.uint64), exp_counts, "counts")
    m = int(exp_counts[0])
    same(r.msg_off[: m + 1].cpu().numpy().view(np.uint64), exp_off, "msg_off")
    same(out[: exp_out.size].cpu().numpy(), exp_out, "out")
    assert bool((out[far.data.size:] == 0xA5).all()) and m >= 20


def test_term_append(codec, far):
    """in_bytes above 2^32, and the source records on both sides of it; the 20 KB record takes
    fifteen frames."""
    lens = np.diff(far.off.astype(np.int64))
    nb = 64 + sum(TA.required(int(x), 1408) for x in lens) + 32
    exp = TA.append_offsets(TA.sentinel(nb), 64, far.data.tobytes(), [int(x) for x in far.off], mtu=1408)
    assert exp["stop"] == TA.END and exp["appended"] == far.n
    guard = 64
    buf = torch.full((guard + nb + guard,), TA.SENTINEL, dtype=torch.uint8, device="cuda")
    version, session, stream, term, base = TA.HEADER
    r = codec.term_append(buf[guard: guard + nb], far.big, far.ro, 64, None, 1408, TA.MAX_LEN,
                          codec.TermHeader(session, stream, term, base, version))
    torch.cuda.synchronize()
    assert int(far.big.numel()) > 2 ** 32
    counts = [int(x) for x in r.counts.cpu().numpy().view(np.uint64)]
    assert counts == [exp["appended"], exp["next"], exp["payload"], exp["stop"]]
    same(r.rec_tail.cpu().numpy().view(np.uint64), np.array(exp["rec_tail"], np.uint64), "rec_tail")
    same(buf.cpu().numpy(), np.frombuffer(TA.sentinel(guard) + exp["block"] + TA.sentinel(guard), np.uint8), "block")
