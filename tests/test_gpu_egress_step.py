"""GPU: egress_commit_step, the subscriber's egress step as one enqueue (term_poll, then the counted
decode, classify, emit and term append, the message count and the frame count never leaving the
device), against the staged pipeline: the existing calls with a host read of counts[4] before the
decode and of totals[0] and the frame table before the append.  The blocks are built with the
term-poll fixtures' tools (termscan_lib.Block, termpoll_lib.pattern): a carry in front, a limit
stop, fragmented messages; the messages are session-framed TopicMessages whose topics name a table
entry, a topic outside the table and a control topic, acks among them.  The step runs twice into
the same buffers, the second block holding fewer messages than the first."""
import numpy as np
import pytest
import torch

import commitfallback_lib as F
import commitsend_lib as C
import sbe_testlib as T
import termpoll_lib as L
import termscan_lib as S
from test_gpu_counted import POISON, fresh_block, gathered, header, raw_bytes
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu
CAPACITY = 256
TERM, SESS = 3, 4


def message(i):
    hd = [b'{"topic":"alpha"}', b'{"topic":"user-%d"}' % i, b'{"topic":"orders_ack"}', b'{"topic":"beta"}', b'{"topic":"gamma"}',
          b'{"topic":12}'][i % 6]
    mid = (b"ack_%d" if i % 7 == 3 else b"id-%d") % i
    if i % 4 == 1:
        rec = T.tm_wire([b"orders", b"SUBSCRIBE", mid, C.P, b"{}"], i)
    elif i % 11 == 5:
        rec = T.ack_wire(b"m%d" % i, b"orders", b"c", i)
    else:
        pay = C.PSEQ if i % 5 == 0 else C.P + b" " * (700 * (i % 9 == 2))
        rec = T.tm_wire([b"orders", b"X", mid, pay, hd], 1_000_000 + i)
    return T.session_wrap(rec, TERM, SESS)


def put(b, msg, mtu=None):
    """The frames of one message: one BEGIN|END frame, or fragments of mtu payload bytes."""
    if mtu is None or len(msg) <= mtu:
        b.frame(msg, 0xC0)
        return
    parts = [msg[k: k + mtu] for k in range(0, len(msg), mtu)]
    for t, p in enumerate(parts):
        b.frame(p, (0x80 if t == 0 else 0) | (0x40 if t == len(parts) - 1 else 0))


def first_block():
    """100 messages, two of every nine in fragments, a padding frame inside; the last message
    stays open (no END): the carry of the next poll."""
    b = S.Block()
    for i in range(100):
        put(b, message(i), 512 if i % 9 == 2 else 96 if i % 9 == 4 else None)
        if i == 50:
            b.pad(96)
    tail = message(100)
    b.frame(tail[:64], 0x80)
    b.frame(tail[64:128], 0x00)
    return b.bytes(), tail


def second_block(tail):
    """The rest of the open message first, then 30 messages of which a limit lets a part through."""
    b = S.Block()
    b.frame(tail[128:], 0x40)
    for i in range(101, 131):
        put(b, message(i), 96 if i % 9 == 2 else None)
    return b.bytes()


class Tables:
    def __init__(self, codec):
        self.ttab = codec.commit_topic_table(F.TOPICS, "cuda")
        self.tid = to_dev(np.asarray(F.TOPIC_IDS, np.uint32), torch.int32)
        self.itab = codec.commit_identifier_table(F.IDENTS, "cuda")
        self.fb = codec.CommitFallback(self.ttab, to_dev(np.frombuffer(F.DEFAULT_IDENT, np.uint8).copy(), torch.uint8),
                                       F.NOW, F.UUID0)


def staged(codec, t, block, start, limit, carry, ingress, ingress_start, frames_cap):
    """The existing calls, the host reading the message count and the frame table in between."""
    p = codec.term_poll(block, start=start, limit=limit, carry=carry, capacity=CAPACITY)
    torch.cuda.synchronize()
    m = int(p.counts[4])  # host read 1
    ro = p.msg_off[: m + 1]
    dec = codec.decode_batch(p.out, ro, mode=codec.DEC_PARSE_MESSAGE, seq=True)
    plan = codec.classify_commits(p.out, ro, dec, t.ttab)
    out = torch.full((frames_cap,), POISON, dtype=torch.uint8, device="cuda")
    fr = codec.emit_commit_offsets(p.out, ro, dec, plan, t.tid, t.itab, out=out, leadership_term_id=TERM,
                                   cluster_session_id=SESS, fallback=t.fb)
    torch.cuda.synchronize()
    dense, off, _ = gathered(fr, m)  # host read 2: totals[0] and the table of frames
    ap = codec.term_append(ingress, to_dev(dense if dense.size else np.zeros(16, np.uint8), torch.uint8),
                           to_dev(off, torch.int64), start=ingress_start, header=header(codec))
    torch.cuda.synchronize()
    return p, m, dec, plan, fr, ap


def carry_of(p, m):
    c = p.counts.cpu().numpy()
    at = int(p.msg_off[m])
    return p.out[at: at + int(c[5])].clone()


def same_step(codec, got, exp, what):
    p, m, dec, plan, fr, ap = exp
    assert np.array_equal(got.polled.counts.cpu().numpy(), p.counts.cpu().numpy()), what
    assert np.array_equal(got.polled.msg_off[: m + 1].cpu().numpy(), p.msg_off[: m + 1].cpu().numpy()), what
    assert np.array_equal(carry_of(got.polled, m).cpu().numpy(), carry_of(p, m).cpu().numpy()), what
    for k in ("status", "flags", "hdr", "ts", "view_off", "view_len"):
        assert np.array_equal(raw_bytes(getattr(got.decoded, k)[:m]), raw_bytes(getattr(dec, k)[:m])), (what, k)
    for k in ("cm", "topic_src", "topic_kind", "topic_off", "topic_len", "topic_idx", "last", "count"):
        a, b = getattr(got.plan, k), getattr(plan, k)
        assert np.array_equal(raw_bytes(a[:m] if k not in ("last", "count") else a), raw_bytes(b)), (what, k)
    tot = fr.totals.cpu().numpy()
    assert np.array_equal(got.frames.totals.cpu().numpy(), tot), what
    assert np.array_equal(got.frames.out_off[: m + 1].cpu().numpy(), fr.out_off.cpu().numpy()), what
    assert np.array_equal(got.frames.status[:m].cpu().numpy(), fr.status.cpu().numpy()), what
    assert np.array_equal(got.frames.emit_idx[: int(tot[0])].cpu().numpy(), fr.emit_idx[: int(tot[0])].cpu().numpy()), what
    assert np.array_equal(got.frames.out[: int(tot[1])].cpu().numpy(), fr.out[: int(tot[1])].cpu().numpy()), what
    assert np.array_equal(got.appended.counts.cpu().numpy(), ap.counts.cpu().numpy()), what
    assert int(ap.counts[0]) == int(tot[0]) and int(ap.counts[3]) == codec.TERM_APPEND_END, what
    assert np.array_equal(got.appended.block.cpu().numpy(), ap.block.cpu().numpy()), what
    return m, tot


def test_two_steps_into_the_same_buffers(codec):
    t = Tables(codec)
    blk1, tail = first_block()
    blk2 = second_block(tail)
    lead = L.carry_bytes(40)  # an open accumulator in front of the first block
    e1 = L.expect(blk1, 0, None, lead)
    assert e1["counts"][3] == S.END and e1["counts"][4] >= 100 and e1["counts"][5] == 128
    assert 110 < e1["counts"][0] < CAPACITY
    limit2 = 12
    e2 = L.expect(blk2, 0, limit2, e1["carry"])
    assert e2["counts"][3] == S.LIMIT and 5 < e2["counts"][4] < 20
    b1, b2 = to_dev(np.frombuffer(blk1, np.uint8).copy(), torch.uint8), to_dev(np.frombuffer(blk2, np.uint8).copy(), torch.uint8)
    frames_cap = codec.commit_fallback_output_bound(CAPACITY, len(blk1) + 64 + CAPACITY * 32, True)
    second_start = 1 << 17
    dlead = to_dev(np.frombuffer(lead, np.uint8).copy(), torch.uint8)

    # the staged pipeline, both steps into one ingress block
    ing_e = fresh_block()
    x1 = staged(codec, t, b1, 0, None, dlead, ing_e, 64, frames_cap)
    ing_e1 = ing_e.clone()
    x2 = staged(codec, t, b2, 0, limit2, carry_of(x1[0], x1[1]), ing_e, second_start, frames_cap)
    assert x1[1] == e1["counts"][4] and x2[1] == e2["counts"][4]
    assert bytes(carry_of(x1[0], x1[1]).cpu().numpy()) == e1["carry"]

    # the step: one enqueue each, no host read between its stages
    ing = fresh_block()
    kw = dict(fallback=t.fb, leadership_term_id=TERM, cluster_session_id=SESS, header=header(codec), capacity=CAPACITY)
    frames_out = torch.full((frames_cap,), POISON, dtype=torch.uint8, device="cuda")
    s1 = codec.egress_commit_step(b1, 0, dlead, t.ttab, t.tid, t.itab, ing, ingress_start=64, frames_out=frames_out, **kw)
    torch.cuda.synchronize()
    x1 = x1[:5] + (type(x1[5])(ing_e1, x1[5].rec_tail, x1[5].counts),)
    m1, tot1 = same_step(codec, s1, x1, "first")
    st = s1.frames.status[:m1].cpu().numpy()
    assert {F.EMITTED, F.EMITTED_JSON, F.HOST, F.NONE} <= set(st.tolist()) and int(tot1[0]) > 20
    carry2 = carry_of(s1.polled, m1)
    s2 = codec.egress_commit_step(b2, 0, carry2, t.ttab, t.tid, t.itab, ing, ingress_start=second_start, limit=limit2,
                                  bufs=s1, **kw)
    torch.cuda.synchronize()
    m2, tot2 = same_step(codec, s2, x2, "second")
    assert m2 < m1 and 0 < int(tot2[0]) < int(tot1[0])
    assert s2.frames.out.data_ptr() == frames_out.data_ptr() and s2.decoded.status.data_ptr() == s1.decoded.status.data_ptr()


def test_a_step_over_an_empty_poll(codec):
    """No message at all (the block starts uncommitted): counts, totals and the append's counts are
    those of empty batches, and the ingress block is not touched."""
    t = Tables(codec)
    blk = to_dev(np.zeros(256, np.uint8), torch.uint8)
    ing = fresh_block()
    s = codec.egress_commit_step(blk, 0, None, t.ttab, t.tid, t.itab, ing, ingress_start=96, fallback=t.fb,
                                 frames_out=torch.full((4096,), POISON, dtype=torch.uint8, device="cuda"), capacity=8,
                                 header=header(codec))
    torch.cuda.synchronize()
    assert int(s.polled.counts[4]) == 0
    assert s.frames.totals.cpu().tolist() == [0, 0, 0] and int(s.frames.out_off[0]) == 0
    assert s.appended.counts.cpu().tolist() == [0, 96, 0, codec.TERM_APPEND_END]
    assert (ing.cpu().numpy() == POISON).all()
    assert s.plan.count.cpu().tolist() == [0] * (len(F.TOPICS) + 2)
