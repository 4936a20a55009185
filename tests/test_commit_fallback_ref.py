"""CPU: sbe_emit_commit_offsets_ex with a fallback, without a GPU.

The expected output is commitfallback_lib.ref_emit (see there).  Its restated quoting is pinned to
the oracle's, one frame is spelled out byte for byte, and where oracle/_ref exists the JSON frames
of the hand table equal the reference's own flyweight with the same put* sequence.  Against the
composition run the per-record functions of csrc/commit_fallback.hpp compiled for the host
(tests/commitfallback/fallback_host_check.cpp: selection, the length rule, frame composition and
the clipping sink), once as a shared object and once inside a stand-alone program built with
-fsanitize=address,undefined.  The quoting helper of the kernels uses device intrinsics and is
checked on the GPU only (test_gpu_commit_fallback.py)."""
import ctypes
import struct
import subprocess

import numpy as np
import pytest

import autocommit_lib as A
import commitfallback_lib as F
import commitsend_lib as C
import sbe_testlib as T

QUOTE_STRINGS = [b"", b"plain", b'q"q', b"b\\s", bytes(range(0x20)), b"\x00", b"a\x00b", b"\x7f/",
                 "é".encode(), "€".encode(), "😀".encode(), "aé€😀z".encode(),
                 b"\xff", b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98", b"\xc0\x80", b"\xe0\x80\x80", b"\xed\xa0\x80",
                 b"\xf0\x80\x80\x80", b"\xf8\x88\x80\x80\x80", b"\x80abc", b"\xc3(", F.ESC_ID, F.DEFAULT_IDENT]


@pytest.mark.parametrize("k", range(len(QUOTE_STRINGS)))
def test_restated_quoting_is_the_oracles(k):
    """Q(s) appears verbatim in the oracle's Order text for an order carrying s (as its side: no
    other field of the text holds it, and the id would be cut at a NUL)."""
    s = QUOTE_STRINGS[k]
    txt = T.oracle_order_json_one([b"u", b"ident", b"BTC", b"USD", s, b"id", b"mid", b"NEW"], 1, 2, 1.0)
    assert b'"side":' + F.quote(s) + b',"token_pair"' in txt, (s, txt)


def _plan(data, off, dec, topics=F.TOPICS):
    return A.ref_classify(data, off, dec, topics)


@pytest.fixture(scope="module")
def hand():
    data, off, dec, seq = C.batch(F.hand_records())
    return data, off, dec, seq, _plan(data, off, dec)


@pytest.fixture(scope="module")
def rnd():
    data, off, dec, seq = C.batch(F.random_records())
    return data, off, dec, seq, _plan(data, off, dec)


def test_exports_and_abi_version():
    import sbecodec
    lib = ctypes.CDLL(sbecodec.LIB_PATH)
    assert hasattr(lib, "sbe_emit_commit_offsets_ex") and hasattr(lib, "sbe_commit_fallback_output_bound")
    assert lib.sbe_abi_version() == 8
    f = lib.sbe_commit_fallback_output_bound
    f.restype, f.argtypes = ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
    assert f(10, 100, 1) == 10 * (1040 + 32) + 10 * (24 + 32) + 100 and f(0, 0, 0) == 0
    assert (sbecodec.CE_EMITTED_JSON, sbecodec.CE_E100_FALLBACK) == (5, 6)
    assert sbecodec.CommitFallback([b"t"], b"c", 1, 2).uuid_ns == 2


def test_hand_table_expectation(hand):
    data, off, dec, seq, plan = hand
    exp = F.ref_emit(data, off, dec, plan, seq=seq, term=5, sess=-9)
    assert list(exp["status"]) == list(F.hand_status())
    # frame 0 spelled out: an id-0 table entry, its identifier z"\x01z escaped in the text, raw in the uuid
    txt = (b'{"action":"COMMIT_OFFSET","messageIdentifier":"z\\"\\u0001z","message_id":"m-gamma",'
           b'"sequence_number":0,"timestamp_nanos":1001,"topic":"gamma"}')
    assert F.frame(exp, 0) == F.spelled_out(5, -9, F.NOW, b'z"\x01z', F.UUID0, txt)
    # the fallback topic (entry 0, id 0): "default" with the entry's identifier
    assert b'"topic":"default"}' in F.frame(exp, 1) and b"commit_offset_client-7_%d" % (F.UUID0 + 1) in F.frame(exp, 1)
    # an unknown plain topic: the default identifier, the flagged sequence number
    f2 = F.frame(exp, 2)
    assert b'"sequence_number":123456789012,' in f2 and b'"topic":"delta"}' in f2
    assert b"commit_offset_" + F.DEFAULT_IDENT + b"_%d" % (F.UUID0 + 2) in f2
    assert b'"messageIdentifier":"client-\\u00e9-0"' in f2
    # "orders" outside the table: the Lite frame with id 3 and the default identifier
    f3 = F.frame(exp, 3)
    assert f3[32:] == struct.pack("<4HIQ", 12, 301, 1, 1, 3, 0) + struct.pack("<H", 8) + b"m-orders" + \
        struct.pack("<H", len(F.DEFAULT_IDENT)) + F.DEFAULT_IDENT
    assert struct.unpack_from("<IQ", F.frame(exp, 4), 40) == (1, 123456789012)
    # negative ts as u64; an unflagged record prints 0 though seq holds a poison there
    assert b'"timestamp_nanos":18446744073709551611,' in F.frame(exp, 9)
    assert b'"sequence_number":0,' in F.frame(exp, 10) and seq[10] == C.POISON
    # every escape class in topic and id
    f7 = F.frame(exp, 7)
    assert b'"topic":"t\\u0001\\u00e9\\ud83d\\ude00/\x7f\\ufffd"}' in f7
    assert b'"message_id":"q\\"b\\\\s\\b\\f\\n\\r\\t\\u0000\\u0001\\u001f\x7f\\u00e9\\u20ac\\ud83d\\ude00\\ufffd\\ufffd"' in f7
    assert int(exp["out_off"][14]) == int(exp["out_off"][13]) == int(exp["out_off"][15])  # E109 and E100: 0 bytes
    assert list(exp["totals"]) == [12, int(exp["out_off"][-1]), 2]


@pytest.mark.skipif(not T.ref_available(), reason="oracle/_ref not built (needs the reference tree)")
def test_sample_against_reference_flyweight(hand):
    """Every JSON frame of the hand table equals the reference's TopicMessage flyweight driven with
    the same put*(const char*, int) sequence (T.ref_publish) on its five strings.  The 1040-byte
    bound cannot be run against it: ref_publish_topic sizes its own buffer."""
    data, off, dec, seq, plan = hand
    exp = F.ref_emit(data, off, dec, plan, seq=seq, session=False)
    k = len(F.TOPIC_IDS)
    seen = 0
    for i in np.nonzero(exp["status"] == F.EMITTED_JSON)[0]:
        i = int(i)
        j = int(plan["topic_idx"][i])
        b = int(off[i]) + int(dec["view_off"][i, 2])
        mid = bytes(data[b: b + int(dec["view_len"][i, 2])])
        if j < k:
            topic, ident = F.TOPICS[j], F.IDENTS[j]
        else:
            tb = int(off[i]) + int(plan["topic_off"][i])
            topic, ident = bytes(data[tb: tb + int(plan["topic_len"][i])]), F.DEFAULT_IDENT
        flagged = dec["flags"][i] & (T.FL_SEQ_KEY | T.FL_SEQ_ESC)
        fields = F.json_fields(topic, ident, mid, int(seq[i]) if flagged else 0, int(dec["ts"][i]), F.UUID0 + i)
        rc, rec = T.ref_publish(fields, F.NOW)
        assert rc == 0 and rec == F.frame(exp, i), i
        seen += 1
    assert seen == 8


def _bound_batch(through):
    """Two records whose JSON records are 1040 and 1041 bytes, the bound reached through the
    identifier (a table entry's) or through the id."""
    if through == "identifier":
        topics, ids = [b"default", b"big0", b"big1"], [0, 0, 0]
        base = 63 + len(F.uuid(b"", F.UUID0)) + F.skeleton_len(b"big0", b"", 0, 77)
        # a plain identifier of L bytes adds L to the uuid and L to the text; the id evens the rest out
        mid = b"m" * (1 + (1040 - base - 1) % 2)
        L = (1040 - base - len(mid)) // 2
        # a quote in place of a plain byte adds nothing to the uuid and 1 to the text
        idents = [b"c", b"I" * L, b"I" * (L - 1) + b'"']
        recs = [T.tm_wire([b"orders", b"X", mid, C.P, b'{"topic":"big%d"}' % r], 77) for r in range(2)]
        return recs, topics, ids, idents, (1040, 1041)
    topics, ids, idents = F.TOPICS, F.TOPIC_IDS, F.IDENTS
    base = 63 + len(F.uuid(F.DEFAULT_IDENT, F.UUID0)) + F.skeleton_len(b"delta", F.DEFAULT_IDENT, 0, 77)
    recs = [T.tm_wire([b"orders", b"X", b"f" * (1040 - base + r), C.P, b'{"topic":"delta"}'], 77) for r in range(2)]
    return recs, topics, ids, idents, (1040, 1041)


@pytest.mark.parametrize("through", ["identifier", "id"])
def test_bound_1040_emits_and_above_throws(through):
    recs, topics, ids, idents, sizes = _bound_batch(through)
    data, off, dec, seq = C.batch(recs)
    plan = _plan(data, off, dec, topics)
    kw = dict(topics=topics, topic_ids=ids, idents=idents, seq=seq, session=True)
    exp = F.ref_emit(data, off, dec, plan, **kw)
    assert list(exp["status"]) == [F.EMITTED_JSON, F.E100], sizes
    assert int(exp["out_off"][1]) == 32 + 1040 and int(exp["out_off"][2]) == 32 + 1040
    F.same(F.chk_emit(data, off, dec, plan, **kw), exp, through)


def wrap_records():
    """A 65535-byte id of 0x01 bytes (its text is 6 * 65535 bytes and the skeleton: the stored
    length wraps), an id that makes the text a multiple of 65536 bytes (an empty payload), and the
    two around it."""
    sk = F.skeleton_len(b"delta", F.DEFAULT_IDENT, 0, 9)
    recs = [T.tm_wire([b"orders", b"X", b"\x01" * 65535, C.P, b'{"topic":"delta"}'], 9)]
    recs += [T.tm_wire([b"orders", b"X", b"w" * (65536 - sk + d), C.P, b'{"topic":"delta"}'], 9) for d in (-1, 0, 1)]
    return recs


def test_u16_wrap():
    data, off, dec, seq = C.batch(wrap_records())
    plan = _plan(data, off, dec)
    exp = F.ref_emit(data, off, dec, plan, seq=seq, session=False)
    sk = F.skeleton_len(b"delta", F.DEFAULT_IDENT, 0, 9)
    u = [len(F.uuid(F.DEFAULT_IDENT, F.UUID0 + i)) for i in range(4)]
    p0 = (6 * 65535 + sk) % 65536
    assert 6 * 65535 + sk > 65536 and 0 < p0 < 900
    assert list(exp["status"]) == [F.EMITTED_JSON, F.E100, F.EMITTED_JSON, F.EMITTED_JSON]
    assert [int(x) for x in np.diff(exp["out_off"])] == [63 + u[0] + p0, 0, 63 + u[2], 63 + u[3] + 1]
    f0 = F.frame(exp, 0)
    full = F.text(b"delta", F.DEFAULT_IDENT, b"\x01" * 65535, 0, 9)
    assert f0.endswith(full[:p0] + b"\x02\x00{}") and f0[-(p0 + 6):-(p0 + 4)] == p0.to_bytes(2, "little")
    assert F.frame(exp, 2).endswith(b"\x00\x00\x02\x00{}") and F.frame(exp, 3).endswith(b"\x01\x00{\x02\x00{}")
    F.same(F.chk_emit(data, off, dec, plan, seq=seq, session=False), exp, "wrap")


CASES = [dict(), dict(session=False), dict(seq=None), dict(mask=True), dict(flags=F.LAST_ONLY),
         dict(cap="minus1"), dict(cap="mid"), dict(cap=0)]


def _kw(case, n, exp_full, seq):
    kw = dict(seq=seq, term=0x0102030405060708, sess=-2)
    kw.update(case)
    if kw.get("mask") is True:
        kw["mask"] = (np.arange(n) % 3 != 1).astype(np.uint8)
    if kw.get("cap") == "minus1":
        kw["cap"] = int(exp_full["out_off"][-1]) - 1
    elif kw.get("cap") == "mid":
        kw["cap"] = int(exp_full["out_off"][n // 2]) + 5
    return kw


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()) or "plain")
@pytest.mark.parametrize("which", ["hand", "rnd"])
def test_device_logic_matches_composition(which, case, hand, rnd):
    data, off, dec, seq, plan = hand if which == "hand" else rnd
    n = off.size - 1
    full = F.ref_emit(data, off, dec, plan, seq=seq, term=0x0102030405060708, sess=-2)
    kw = _kw(case, n, full, seq)
    exp = F.ref_emit(data, off, dec, plan, **kw)
    got = F.chk_emit(data, off, dec, plan, **kw)
    F.same(got, exp, (which, case))
    assert got["out"].size == exp["out"].size
    if "cap" in case:  # the full layout whatever the capacity
        assert np.array_equal(exp["out_off"], full["out_off"]) and np.array_equal(exp["totals"], full["totals"])
        assert (exp["status"] == F.OVERFLOW).any()


def test_random_batch_covers_every_status(rnd):
    """The distribution the GPU test relies on, shown by the composition alone: every status at
    least once (OVERFLOW under a short capacity) and at least a tenth of the records JSON frames."""
    data, off, dec, seq, plan = rnd
    n = off.size - 1
    exp = F.ref_emit(data, off, dec, plan, seq=seq)
    cnt = np.bincount(exp["status"], minlength=7)
    assert all(cnt[s] >= 1 for s in (F.NONE, F.EMITTED, F.HOST, F.E109, F.EMITTED_JSON, F.E100)), cnt
    assert cnt[F.EMITTED_JSON] * 10 >= n, cnt
    short = F.ref_emit(data, off, dec, plan, seq=seq, cap=int(exp["out_off"][n // 2]) + 5)
    assert (short["status"] == F.OVERFLOW).any()
    js = exp["status"] == F.EMITTED_JSON
    assert (plan["topic_idx"][js] == 0).any() and (plan["topic_idx"][js] == 4).any() and \
        (plan["topic_idx"][js] == A.UNKNOWN).any()
    named = (exp["status"] == F.EMITTED) & (plan["topic_idx"] == A.UNKNOWN)
    assert named.any()  # "orders" outside the table: Lite
    host = plan["topic_idx"][exp["status"] == F.HOST]
    assert (host == A.HOST).any() and (host == A.UNKNOWN).any()  # numbers; escaped unknown strings
    # without a fallback the same batch leaves all of these to the host
    plain = C.ref_emit(data, off, dec, plan, F.TOPIC_IDS, F.IDENTS, seq=seq)
    assert int(plain["totals"][2]) == int(exp["totals"][2]) + cnt[F.EMITTED_JSON] + cnt[F.E100] + int(named.sum()) + \
        int(((exp["status"] == F.E109) & (plan["topic_idx"] == A.UNKNOWN)).sum())


def test_last_only_filters_table_entries_only(rnd):
    data, off, dec, seq, plan = rnd
    exp = F.ref_emit(data, off, dec, plan, seq=seq, flags=F.LAST_ONLY)
    tab = plan["topic_idx"] < len(F.TOPICS)
    emitted = (exp["status"] == F.EMITTED) | (exp["status"] == F.EMITTED_JSON)
    assert set(np.nonzero(emitted & tab)[0]) <= {int(x) for x in plan["last"]}
    assert (exp["status"][int(plan["last"][0])] == F.EMITTED_JSON) and (emitted & ~tab).sum() > 10
    with pytest.raises(ValueError, match="SBE_EINVAL"):
        F.chk_emit(data, off, dec, plan, flags=F.LAST_ONLY, mask=np.ones(off.size - 1, np.uint8))


def test_table_offsets_are_clamped(hand):
    data, off, dec, seq, plan = hand
    arena, toff = A.topic_table(F.TOPICS)
    bad = toff.copy()
    bad[5], bad[6] = 0xFFFFFFF0, 12  # entry 4 ("gamma") runs to the clamp, entry 5 is reversed: empty
    lens = np.minimum(bad, 4096)
    topics = [bytes(arena[int(lens[j]): int(lens[j + 1])]) if lens[j + 1] > lens[j] else b"" for j in range(len(F.TOPICS))]
    assert len(topics[4]) == 4096 - int(toff[4]) and topics[5] == b""
    exp = F.ref_emit(data, off, dec, plan, topics=topics, seq=seq)
    assert exp["status"][0] == F.E100  # a 4 KiB topic does not fit 1040 bytes
    F.same(F.chk_emit(data, off, dec, plan, topics=(arena, bad), seq=seq), exp, "clamp")


def test_host_build_under_sanitizers(tmp_path, hand, rnd):
    """The same host build inside a stand-alone program with AddressSanitizer and UBSan: every input
    array in a heap block of exactly its size, `out` of exactly the capacity."""
    prog = F._make("fallback_sanitize")
    files = []
    wdata, woff, wdec, wseq = C.batch(wrap_records())
    wrap = (wdata, woff, wdec, wseq, _plan(wdata, woff, wdec))
    for which, (data, off, dec, seq, plan) in (("hand", hand), ("rnd", rnd), ("wrap", wrap)):
        n = off.size - 1
        full = F.ref_emit(data, off, dec, plan, seq=seq, term=0x0102030405060708, sess=-2)
        for c, case in enumerate(CASES if which != "wrap" else CASES[:2]):
            kw = _kw(case, n, full, seq)
            exp = F.ref_emit(data, off, dec, plan, **kw)
            path = tmp_path / f"{which}{c}.bin"
            F.write_case(path, data, off, dec, plan, exp, **kw)
            files.append(str(path))
    r = subprocess.run([prog] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(files)} cases ok" in r.stdout
