"""CPU: the auto-commit decision (sbe_classify_commits) without a GPU.

Three things are compared: the hand table's expectations (autocommit_lib.HAND, the reference's
clauses and extraction branches spelled out case by case), the restatement
tests/autocommit/commit_ref.cpp (a tree-building reader with jsoncpp 1.9.5 semantics and the three
reference functions on top) and the device classifier of csrc/commit_class.hpp compiled for the
host.  jsoncpp is absent from this image, so parity with the library itself is unpinned; the
restatement's reader is pinned to the project's oracle through _sequence_number (orc_seq_eval)."""
import random

import numpy as np
import pytest

import autocommit_lib as A
import sbe_testlib as T
import test_oracle_seqnum as S


def _batch(recs):
    data, off = T.pack_records(recs)
    return data, off, T.oracle_decode(data, off, T.DEC_PARSE)


def _same(a, b, what):
    for k in A.KEYS:
        bad = np.nonzero(a[k] != b[k])[0]
        assert bad.size == 0, (what, k, bad[:5], a[k][bad[:5]], b[k][bad[:5]])


@pytest.fixture(scope="module")
def hand():
    return _batch(A.hand_records())


def test_restatement_reader_matches_oracle_on_hand_cases():
    for doc, exp in S.HAND_CASES:
        d = doc.encode() if isinstance(doc, str) else doc
        assert A.ref_seq(d) == exp == T.oracle_seq_eval(d), doc
    ok = '{"_sequence_number": 1, "a": ' + "[" * 999 + "]" * 999 + "}"
    deep = '{"_sequence_number": 1, "a": ' + "[" * 1000 + "]" * 1000 + "}"
    assert A.ref_seq(ok.encode()) == 1 and A.ref_seq(deep.encode()) == 0


def test_restatement_reader_matches_oracle_on_random_and_mangled_documents():
    for doc in S._docs(0xD0C, 12000):
        assert A.ref_seq(doc) == T.oracle_seq_eval(doc), doc


def test_hand_table_restatement(hand):
    data, off, dec = hand
    assert (dec["status"] == 0).all()
    A.check_hand(A.ref_classify(data, off, dec, A.TOPICS), data, off)


def test_hand_table_device_logic(hand):
    data, off, dec = hand
    out = A.chk_classify(data, off, dec, A.TOPICS)
    A.check_hand(out, data, off)
    _same(out, A.ref_classify(data, off, dec, A.TOPICS), "hand")


def test_hand_table_counts(hand):
    data, off, dec = hand
    out = A.ref_classify(data, off, dec, A.TOPICS)
    k = len(A.TOPICS)
    com = out["cm"] == A.COMMIT
    for j in range(k):
        sel = np.nonzero(com & (out["topic_idx"] == j))[0]
        assert out["count"][j] == sel.size
        assert out["last"][j] == (sel[-1] if sel.size else 2**64 - 1)
    assert out["count"][k] == (com & (out["topic_idx"] == A.UNKNOWN)).sum()
    assert out["count"][k + 1] == (com & (out["topic_idx"] == A.HOST)).sum()
    assert out["count"][3] == 0 and out["last"][3] == 2**64 - 1  # the duplicate entry: the first one wins
    assert not (~com & (out["topic_idx"] != A.UNKNOWN)).any()


def test_fallback_topic_that_is_a_control_name():
    recs = [T.tm_wire([b"t", ty, b"m1", pl, b"{}"], 5) for ty, pl in
            ((b"X", A.P), (b"REPLAY_COMPLETE", b""), (b"X", b'"REPLAY_COMPLETE"'), (b"X", b""))]
    data, off, dec = _batch(recs)
    for fb, exp in ((b"_control", [A.SKIP_CONTROL, A.COMMIT, A.COMMIT, A.SKIP_CONTROL]),
                    (b"_ack", [A.SKIP_TOPIC] * 4), (b"_subscriptions", [A.SKIP_TOPIC] * 4),
                    (b"_controls", [A.COMMIT, A.SKIP_EMPTY, A.COMMIT, A.SKIP_EMPTY])):
        r = A.ref_classify(data, off, dec, [fb, b"x"])
        assert list(r["cm"]) == exp, fb
        assert (r["topic_src"] == A.FALLBACK).all() and (r["topic_len"] == 0).all()
        _same(A.chk_classify(data, off, dec, [fb, b"x"]), r, fb)


def test_other_record_kinds():
    tm = T.tm_wire([b"t", b"X", b"m1", A.P, b'{"topic":"alpha"}'], 5)
    recs = [T.ack_wire(b"id1", b"orders", b"c", 5), T.session_event(1, 9, 7, 1, 0, b'{"topic":"alpha"}'),
            T.session_wrap(tm), b"", b"\x01", T.hdr_bytes(16, 77, 1, 1) + b"\0" * 16,
            tm[:-3]]  # headers cut short: SBE_FL_HEADERS_E100, headers = ""
    data, off, dec = _batch(recs)
    assert list(dec["status"][:3]) == [1, 2, 0]  # SBE_ST_ACK, SBE_ST_SESSION_EVENT, SBE_ST_TM
    assert dec["status"][6] == 0 and dec["flags"][6] & 0x4
    r = A.ref_classify(data, off, dec, A.TOPICS)
    assert list(r["cm"]) == [A.SKIP_TYPE, A.NO_ID, A.COMMIT, A.NOT_PARSED, A.NOT_PARSED, A.NOT_PARSED, A.COMMIT]
    assert list(r["topic_src"]) == [A.NONE, A.NONE, A.HEADERS, A.NONE, A.NONE, A.NONE, A.FALLBACK]
    assert r["topic_idx"][2] == 1 and r["topic_idx"][6] == 0
    b = int(off[2]) + int(r["topic_off"][2])
    assert bytes(data[b: b + 5]) == b"alpha"
    _same(A.chk_classify(data, off, dec, A.TOPICS), r, "kinds")


RANDOM_SEED, RANDOM_N = 0xAC01, 3000


def test_random_batch_covers_every_code():
    """The distribution the GPU test relies on, shown by the restatement alone."""
    data, off, dec = _batch(A.random_records(RANDOM_N, RANDOM_SEED))
    r = A.ref_classify(data, off, dec, A.TOPICS)
    cm = np.bincount(r["cm"], minlength=8)
    src = np.bincount(r["topic_src"], minlength=5)
    assert all(cm[c] >= 100 for c in (0, 2, 3, 4, 5, 6, 7)), cm
    assert all(src[s] >= 100 for s in (1, 2, 3, 4)), src
    assert (dec["flags"] & 0x4).any() and (dec["status"] >= 16).any()


@pytest.mark.parametrize("seed", [RANDOM_SEED, 7, 8])
def test_random_batches_device_logic_matches_restatement(seed):
    data, off, dec = _batch(A.random_records(RANDOM_N, seed))
    _same(A.chk_classify(data, off, dec, A.TOPICS), A.ref_classify(data, off, dec, A.TOPICS), seed)


def test_random_documents_device_logic_matches_restatement():
    """The seqnum suite's random, mangled and byte-soup documents as headers and payloads."""
    docs = S._docs(0xD0D, 6000)
    r = random.Random(3)
    soup = [bytes(r.choice(b'topicmesag\\"{}[]:,/*\n u0067') for _ in range(r.randrange(0, 60))) for _ in range(3000)]
    docs = [d for d in docs + soup if len(d) < 60000]
    recs = [T.tm_wire([b"t", b"X", b"m1", docs[i], docs[(i * 7 + 3) % len(docs)]], i) for i in range(len(docs))]
    data, off, dec = _batch(recs)
    _same(A.chk_classify(data, off, dec, A.TOPICS), A.ref_classify(data, off, dec, A.TOPICS), "docs")


def test_table_offsets_are_clamped():
    data, off, dec = _batch([T.tm_wire([b"t", b"X", b"m1", A.P, b'{"topic":"alpha"}'], 5)])
    arena, toff = A.topic_table([b"orders", b"alpha"])
    bad = toff.copy()
    bad[1], bad[2] = 0xFFFFFFF0, 5  # past the arena, and an end before its start
    r = A.ref_classify(data, off, dec, (arena, bad))
    assert r["cm"][0] == A.COMMIT and r["topic_idx"][0] == A.UNKNOWN
    _same(A.chk_classify(data, off, dec, (arena, bad)), r, "clamp")
