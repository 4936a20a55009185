"""CPU: the oracle restatement (oracle/sbe_oracle.c) and the predicate model (tests/select_lib.py)
against the reference's own compiled codec source (oracle/_ref/libsbe_ref_src.so: its
src/sbe_encoder.cpp behind oracle/ref_sources.cpp): MessageParser::parse_message with every
ParseResult field, the _sequence_number lookup, the four ParseResult predicates, classify_topic and
SBEEncoder::encode_topic_message.  Every comparison is exact.  Skipped where the library was not
built (it needs the reference tree).

The corpus, its seed and the class counts measured for it are in tests/refsrc_lib.py; the
conditions that keep these comparisons from hiding a failure (precondition, 14 outcome classes of
at least 20 records each) are asserted here from the reference's verdicts."""
import numpy as np
import pytest

import refsrc_lib as R
import sbe_testlib as T
import select_lib as S
from test_oracle_seqnum import _docs
from test_oracle_vs_ref import rand_fields

pytestmark = pytest.mark.skipif(not T.refsrc_available(),
                                reason="oracle/_ref/libsbe_ref_src.so not built (needs the reference tree)")


def test_conditions():
    counts = R.check_conditions()
    print(counts)
    assert len(counts) == 14 and len(R.records()) >= 8000


def test_parse_message_all_fields():
    R.check_conditions()
    recs = R.records()
    res, _, kept = R.reference()
    data, off = R.packed()
    dec = T.oracle_decode(data, off, T.DEC_PARSE)
    seq = T.oracle_seq_batch(data, off, dec)
    for i in kept:
        got = R.with_seq(recs[i], T.row(dec, i), seq[i])
        assert got == res[i], (i, recs[i][:64].hex(), R.diff(got, res[i]))
    assert not (dec["status"] == T.ST_ERR_DIRECT_TEMPLATE).any()  # unreachable through parse_message


def test_sequence_number_lookup():
    """The reference's own lookup (four locations, seq > 0 fall-through, conversion order, stoull,
    catch) on the seqnum suite's hand cases and 8000 of its random documents, as TopicMessage
    payloads.  The JSON reader under it is the project's (oracle/refsrc_standin)."""
    docs = [d for d in _docs(0x5EC, 8000) if len(d) <= 65000]
    assert len(docs) >= 8000
    nonzero = 0
    for k, d in enumerate(docs):
        rec = T.tm_wire([b"t", b"T", b"u", d, b"{}"], k + 1)
        r = T.ref_parse_message(rec)
        assert r["success"] and r["payload"] == d
        assert r["sequence_number"] == T.oracle_seq_eval(d), d
        nonzero += r["sequence_number"] != 0
    assert nonzero >= 1000


@pytest.mark.parametrize("which", ["edge", "mutated", "corpus"])
def test_predicates_and_topic_class(which):
    if which == "edge":
        names, data, off, dec = S.edge_case(S.window())
        keep = range(len(names))
    elif which == "mutated":
        data, off, dec = S.mutated_case(3000, 0x77)
        keep = range(len(off) - 1)
    else:
        data, off = R.packed()
        dec = T.oracle_decode(data, off, T.DEC_PARSE)
        keep = R.reference()[2]
    exp = S.model(data, off, dec)
    pred, tc = R.ref_model(R.split(data, off), dec)
    for i in keep:
        assert exp["pred"][i] == pred[i] and exp["topic_class"][i] == tc[i], (which, i, int(exp["pred"][i]), int(pred[i]))
    # each predicate is seen true and false (mixed_records, under "mutated", holds no SessionEvent
    # and nothing that is not a topic message)
    bits = (S.PR_ACKNOWLEDGMENT, S.PR_ORDER_MESSAGE) if which == "mutated" else \
        (S.PR_SESSION_EVENT, S.PR_TOPIC_MESSAGE, S.PR_ACKNOWLEDGMENT, S.PR_ORDER_MESSAGE)
    for bit in bits:
        on = sum(1 for i in keep if pred[i] & bit)
        assert on >= 10 and len(keep) - on >= 10, (which, bit, on)


def test_classify_topic_names():
    for t in S.TOPICS_ORDERS + S.TOPICS_CONTROL + (b"", b"order", b"orderss", b"_ack\0", b"Orders", b"default"):
        assert T.ref_classify_topic(t) == S.classify_topic(t), t


def test_encode_topic_message():
    rng = np.random.default_rng(2024)  # the 400 records of test_oracle_vs_ref.test_encode_random_vs_ref
    recs = [rand_fields(rng) for _ in range(400)]
    ts = rng.integers(1, 2**63, len(recs), dtype=np.uint64)
    for ln in (65534, 65535, 65536):
        for k in range(5):
            f = [b"a", b"b", b"c", b"d", b"e"]
            f[k] = bytes(rng.integers(0, 256, ln, dtype=np.uint8))
            recs.append(f)
    ts = np.concatenate([ts, np.arange(1, 16, dtype=np.uint64)])
    L = np.array([[len(f) for f in r] for r in recs], np.uint32)
    arena = np.frombuffer(b"".join(b"".join(r) for r in recs), np.uint8)
    out, off, st = T.oracle_encode(arena, L, ts, flags=T.ENC_REF_TRUNCATE8)
    names = [b"topicLength", b"messageTypeLength", b"uuidLength", b"payloadLength", b"headersLength"]
    n_e109 = 0
    for i, r in enumerate(recs):
        rc, ref = T.ref_encode_topic_message(r, int(ts[i]))
        if rc:  # E109: the exception's text names the field the oracle's status numbers
            assert 1 <= st[i] <= 5 and ref.startswith(names[int(st[i]) - 1]) and b"E109" in ref, (i, st[i], ref)
            assert off[i + 1] == off[i]
            n_e109 += 1
        else:
            assert st[i] == 0 and bytes(out[off[i]:off[i + 1]]) == ref, i
    assert n_e109 == 10


def test_host_mirror_byte_helpers(tmp_path):
    """The host mirror's helpers that need no device (MessageParser::get_message_type,
    extract_correlation_id, SBEUtils::is_valid_sbe_message, extract_readable_strings,
    get_session_event_code_string) against the reference's, as lines of oracle/parse_line.hpp, on
    the hand table and the first 1500 corpus records."""
    recs = R.records()[: len(R.hand_table()) + 1500]
    got = R.mirror_lines(recs, "bytes", tmp_path)
    R.same_lines(got, [T.ref_describe(r, T.DESC_BYTES) for r in recs], recs, "bytes")
    assert len({ln.split(" ")[0] for ln in got}) >= 8 and sum("valid=1" in ln for ln in got) >= 300
