"""GPU: the device decode, its fused _sequence_number, sbe_order_select, the REF-mode encode and the
host mirror against the reference's own compiled codec source (oracle/_ref/libsbe_ref_src.so, built
by build() where the reference tree is present: its src/sbe_encoder.cpp behind
oracle/ref_sources.cpp), live and with no oracle in between.  Every comparison is exact.

The records are those of tests/refsrc_lib.py (the hand table, then 8000 seeded records of five
kinds) and go to the device as one batch, so a mutated record sits in a 64-record tile among valid
ones of other kinds.  The conditions that keep a comparison from hiding a failure (at most 5 % left
out because the reference read past them, 14 outcome classes of at least 20 records each) are
asserted from the reference's verdicts, never from the device's."""
import numpy as np
import pytest
import torch

import contract_lib as C
import refsrc_lib as R
import sbe_testlib as T
import select_lib as S
from test_gpu_order_select import dev
from test_gpu_parity import gpu_encode
from test_gpu_vs_ref import encode_inputs
from test_oracle_seqnum import HAND_CASES

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not T.refsrc_available(),
                                 reason="oracle/_ref/libsbe_ref_src.so not built (needs the reference tree)")]


@pytest.mark.parametrize("shift", [0, 1, 15])
def test_parse_message_all_fields(codec, shift):
    """decode_batch(DEC_PARSE_MESSAGE) with the fused sequence number: all 17 ParseResult fields of
    every kept record.  The call wants its input at 16 bytes; contract_lib.placed puts it at exactly
    that and no better, and a byte shift is a record of `shift` bytes in front (its row is dropped),
    which moves every record and every tile's first byte by `shift`."""
    R.check_conditions()
    recs = R.records()
    res, _, kept = R.reference()
    data, off = T.pack_records([b"\0" * shift] + list(recs)) if shift else R.packed()
    lead = 1 if shift else 0
    assert len(recs) // 64 >= 100 and data.nbytes < 2 << 20
    dec = codec.decode_batch(C.placed(data, 16), C.placed(off, 8), mode=codec.DEC_PARSE_MESSAGE, seq=True)
    torch.cuda.synchronize()
    got = {k: v[lead:] for k, v in dec.numpy().items()}
    seq = dec.seq.cpu().numpy().view(np.uint64)[lead:]
    for i in kept:
        pr = R.with_seq(recs[i], T.row(got, i), seq[i])
        assert pr == res[i], (i, recs[i][:64].hex(), R.diff(pr, res[i]))
    assert not (got["status"] == T.ST_ERR_DIRECT_TEMPLATE).any()
    assert sum(1 for i in kept if res[i]["sequence_number"]) >= 20


@pytest.mark.parametrize("which", ["corpus", "edge"])
def test_order_select_predicates(codec, which):
    """sbe_order_select's pred and topic_class over the device's own decode against the
    reference's four predicates and classify_topic."""
    if which == "corpus":
        R.check_conditions()
        data, off = R.packed()
        keep = R.reference()[2]
    else:
        names, data, off, _ = S.edge_case(codec.order_select_window())
        keep = range(len(names))
    d, ro = dev(data), dev(off)
    ddec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE)
    pred, tc = R.ref_model(R.split(data, off), ddec.numpy())
    for shift in (0, 1, 15):  # sbe_order_select takes its input at any byte
        got = codec.order_select(C.placed(data, shift) if shift else d, ro, ddec).numpy()
        bad = [(i, int(got["pred"][i]), int(pred[i]), int(got["topic_class"][i]), int(tc[i])) for i in keep
               if got["pred"][i] != pred[i] or got["topic_class"][i] != tc[i]]
        assert not bad, (which, shift, len(bad), bad[:8])
    for bit in (S.PR_SESSION_EVENT, S.PR_TOPIC_MESSAGE, S.PR_ACKNOWLEDGMENT, S.PR_ORDER_MESSAGE):
        on = sum(1 for i in keep if pred[i] & bit)
        assert on >= 10 and len(keep) - on >= 10, (which, bit, on)
    assert all(sum(1 for i in keep if tc[i] == c) >= 4 for c in (S.TC_UNKNOWN, S.TC_ORDERS, S.TC_CONTROL))


def test_sequence_numbers_hand_cases(codec):
    """The seqnum suite's hand cases as one batch: the decode's fused evaluation and the
    stand-alone sbe_seqnum_kernel against the reference's own lookup."""
    docs = [(d.encode() if isinstance(d, str) else d) for d, _ in HAND_CASES]
    recs = [T.tm_wire([b"orders", b"T", b"id", p, b"{}"], k + 1) for k, p in enumerate(docs)]
    exp = np.array([T.ref_parse_message(r)["sequence_number"] for r in recs], np.uint64)
    assert (exp == np.array([e for _, e in HAND_CASES], np.uint64)).all() and int((exp != 0).sum()) >= 40
    data, off = T.pack_records(recs)
    d, ro = dev(data), dev(off)
    dec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE, seq=True)
    alone = codec.eval_sequence_numbers(d, ro, dec)
    torch.cuda.synchronize()
    for name, s in (("fused", dec.seq), ("stand-alone", alone)):
        got = s.cpu().numpy().view(np.uint64)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (name, [(docs[i], int(got[i]), int(exp[i])) for i in bad[:5]])


def test_encode_topic_message(codec):
    """encode_topic_batch under ENC_REF_TRUNCATE8 against SBEEncoder::encode_topic_message itself on
    the 2000 records of test_gpu_vs_ref.encode_inputs()."""
    recs, ts, L, arena, long_at = encode_inputs()
    out, off, st = gpu_encode(codec, arena, L, ts, flags=T.ENC_REF_TRUNCATE8)
    out = out.tobytes()
    names = [b"topicLength", b"messageTypeLength", b"uuidLength", b"payloadLength", b"headersLength"]
    n_e109 = 0
    for i, r in enumerate(recs):
        rc, ref = T.ref_encode_topic_message(r, T._i64(ts[i]))
        got = out[int(off[i]):int(off[i + 1])]
        if rc:
            assert 1 <= st[i] <= 5 and ref.startswith(names[int(st[i]) - 1]) and b"E109" in ref and got == b"", (i, st[i], ref)
            n_e109 += 1
        else:
            assert st[i] == 0 and got == ref, (i, int(st[i]), len(got), len(ref))
    assert n_e109 == sum(1 for _, ln in long_at.values() if ln > 65534) >= 10


def test_host_mirror_lines(codec, tmp_path):
    """The host mirror (tests/cpp/test_parse_lines.cpp) against the reference, as lines of
    oracle/parse_line.hpp: MessageParser::parse_message, ParseResult::get_description, the predicates,
    is_acknowledgment_for and the byte helpers one record at a time on the hand table and 200 corpus
    records; MessageParser::parse_batch over all records."""
    R.check_conditions()
    recs = R.records()
    kept = set(R.reference()[2])
    few = [r for i, r in enumerate(recs[: len(R.hand_table()) + 200]) if i in kept]
    R.same_lines(R.mirror_lines(few, "single", tmp_path), [T.ref_describe(r) for r in few], few, "single")
    got = R.mirror_lines(recs, "batch", tmp_path)
    exp = [T.ref_describe(r, T.DESC_RESULT) for r in recs]
    idx = sorted(kept)
    R.same_lines([got[i] for i in idx], [exp[i] for i in idx], [recs[i] for i in idx], "batch")
