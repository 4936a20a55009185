"""CPU: sbe_emit_commit_offsets without a GPU.

The expected output is commitsend_lib.ref_emit, a composition of autocommit_lib.ref_classify (the
plan), the oracle's orc_encode_lite_batch (template 301) and the session header bytes of
orc_encode_session_batch.  Against it run the device sizing and writing functions of
csrc/commit_emit.hpp compiled for the host (tests/commitsend/emit_host_check.cpp), once as a
shared object and once inside a stand-alone program built with -fsanitize=address,undefined."""
import struct
import subprocess

import numpy as np
import pytest

import autocommit_lib as A
import commitsend_lib as C
import sbe_testlib as T


def _plan(data, off, dec, topics=C.TOPICS):
    return A.ref_classify(data, off, dec, topics)


@pytest.fixture(scope="module")
def hand():
    data, off, dec, seq = C.batch(C.hand_records())
    return data, off, dec, seq, _plan(data, off, dec)


@pytest.fixture(scope="module")
def rnd():
    data, off, dec, seq = C.batch(C.random_records())
    return data, off, dec, seq, _plan(data, off, dec)


def _frame(out, off, i):
    return bytes(out[int(off[i]): int(off[i + 1])])


def test_hand_table_expectation(hand):
    data, off, dec, seq, plan = hand
    exp = C.ref_emit(data, off, dec, plan, C.TOPIC_IDS, C.IDENTS, seq=seq, term=5, sess=-9)
    assert list(exp["status"]) == list(C.hand_status())
    # frame 1 spelled out: session header, {12,301,1,1}, topicId, sequence, the two strings
    f = _frame(exp["out"], exp["out_off"], 1)
    assert f == struct.pack("<4Hqqq", 24, 1, 111, 8, 5, -9, 0) + struct.pack("<4HIQ", 12, 301, 1, 1, 22, 123456789012) + \
        struct.pack("<H", 7) + b"m-alpha" + struct.pack("<H", 9) + b"sub-alpha"
    # an unflagged record carries sequence 0, not the poison decode left in seq
    f = _frame(exp["out"], exp["out_off"], 0)
    assert struct.unpack_from("<Q", f, 32 + 12)[0] == 0 and seq[0] == C.POISON
    assert _frame(exp["out"], exp["out_off"], 2).endswith(b"m-beta\x00\x00")
    assert struct.unpack_from("<I", _frame(exp["out"], exp["out_off"], 7), 32 + 8)[0] == 0x80000001
    assert int(exp["out_off"][14]) == int(exp["out_off"][13])  # the 65535-byte id: 0 bytes
    assert int(exp["out_off"][15] - exp["out_off"][14]) == 32 + 24 + 65534 + 9
    assert list(exp["totals"]) == [8, int(exp["out_off"][-1]), 3]


@pytest.mark.skipif(not T.ref_available(), reason="oracle/_ref not built (needs the reference tree)")
def test_sample_against_reference_flyweight(hand):
    data, off, dec, seq, plan = hand
    exp = C.ref_emit(data, off, dec, plan, C.TOPIC_IDS, C.IDENTS, seq=seq, session=False)
    for i in exp["emit_idx"]:
        i = int(i)
        j = int(plan["topic_idx"][i])
        b = int(off[i]) + int(dec["view_off"][i, 2])
        mid = bytes(data[b: b + int(dec["view_len"][i, 2])])
        flagged = dec["flags"][i] & (T.FL_SEQ_KEY | T.FL_SEQ_ESC)
        rc, rec = T.ref_lite_encode(301, [mid, C.IDENTS[j]], C.TOPIC_IDS[j], int(seq[i]) if flagged else 0)
        assert rc == 0 and rec == _frame(exp["out"], exp["out_off"], i), i


CASES = [dict(), dict(session=False), dict(seq=None), dict(mask=True), dict(flags=C.LAST_ONLY),
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
    full = C.ref_emit(data, off, dec, plan, C.TOPIC_IDS, C.IDENTS, seq=seq, term=0x0102030405060708, sess=-2)
    kw = _kw(case, n, full, seq)
    exp = C.ref_emit(data, off, dec, plan, C.TOPIC_IDS, C.IDENTS, **kw)
    got = C.chk_emit(data, off, dec, plan, C.TOPIC_IDS, C.IDENTS, **kw)
    C.same(got, exp, (which, case))
    assert got["out"].size == exp["out"].size
    if "cap" in case:  # the full layout whatever the capacity
        assert np.array_equal(exp["out_off"], full["out_off"]) and np.array_equal(exp["totals"], full["totals"])
        assert (exp["status"] == C.OVERFLOW).any()


def test_random_batch_covers_every_status(rnd):
    """The distribution the GPU test relies on, shown by the composition alone."""
    data, off, dec, seq, plan = rnd
    exp = C.ref_emit(data, off, dec, plan, C.TOPIC_IDS, C.IDENTS, seq=seq)
    cnt = np.bincount(exp["status"], minlength=5)
    assert all(cnt[s] >= 1 for s in (C.NONE, C.EMITTED, C.HOST, C.E109)), cnt
    assert cnt[C.EMITTED] * 10 >= off.size - 1, cnt
    idx = plan["topic_idx"][exp["status"] == C.HOST]
    assert (idx == 4).any() and (idx == A.UNKNOWN).any() and (idx == A.HOST).any()  # id 0, unknown, host-resolved
    assert not (plan["topic_idx"] == 3).any()  # the duplicate entry never matches
    flagged = (dec["flags"] & (T.FL_SEQ_KEY | T.FL_SEQ_ESC)) != 0
    assert (exp["status"][~flagged] == C.EMITTED).any()


def test_last_only_emits_one_frame_per_entry(rnd):
    data, off, dec, seq, plan = rnd
    exp = C.ref_emit(data, off, dec, plan, C.TOPIC_IDS, C.IDENTS, seq=seq, flags=C.LAST_ONLY)
    want = sorted(int(plan["last"][j]) for j in range(len(C.TOPICS))
                  if C.TOPIC_IDS[j] and plan["last"][j] != 2**64 - 1 and dec["view_len"][int(plan["last"][j]), 2] <= 65534)
    assert [int(i) for i in exp["emit_idx"]] == want and 2 <= len(want) <= len(C.TOPICS)
    with pytest.raises(ValueError, match="SBE_EINVAL"):  # LAST_ONLY together with a mask
        C.chk_emit(data, off, dec, plan, C.TOPIC_IDS, C.IDENTS, flags=C.LAST_ONLY, mask=np.ones(off.size - 1, np.uint8))


def test_identifier_offsets_are_clamped(hand):
    data, off, dec, seq, plan = hand
    arena, ioff = C.ident_table(C.IDENTS)
    bad = ioff.copy()
    bad[2], bad[3] = 0xFFFFFFF0, 12  # entry 1 runs to the clamp, entry 2 is reversed: empty
    lens = np.minimum(bad, 4096)
    idents = [bytes(arena[int(lens[j]): int(lens[j + 1])]) if lens[j + 1] > lens[j] else b"" for j in range(len(C.IDENTS))]
    assert len(idents[1]) == 4096 - 8 and idents[2] == b""
    exp = C.ref_emit(data, off, dec, plan, C.TOPIC_IDS, idents, seq=seq)
    C.same(C.chk_emit(data, off, dec, plan, C.TOPIC_IDS, (arena, bad), seq=seq), exp, "clamp")


def _write_case(path, data, off, dec, plan, seq, mask, flags, session, term, sess, cap, exp):
    n, k = off.size - 1, len(C.TOPIC_IDS)
    arena, ioff = C.ident_table(C.IDENTS)
    cap = int(exp["out_off"][-1]) if cap is None else cap
    head = np.array([0x3130454354494d43, n, k, data.size, flags, int(session), term % 2**64, sess % 2**64, cap,
                     seq is not None, mask is not None, exp["out"].size], np.uint64)
    parts = [head, data.astype(np.uint8), off.astype(np.uint64), dec["status"], dec["flags"],
             dec["view_off"].astype(np.uint32), dec["view_len"].astype(np.uint32)]
    parts += [] if seq is None else [seq.astype(np.uint64)]
    parts += [plan["cm"], plan["topic_idx"].astype(np.uint32), plan["last"].astype(np.uint64),
              np.asarray(C.TOPIC_IDS, np.uint32), arena, ioff.astype(np.uint32)]
    parts += [] if mask is None else [mask.astype(np.uint8)]
    parts += [exp["out_off"], exp["status"], exp["totals"], exp["emit_idx"], exp["out"]]
    with open(path, "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p).tobytes())


def test_host_build_under_sanitizers(tmp_path, hand, rnd):
    """The same host build inside a stand-alone program with AddressSanitizer and UBSan: every input
    array in a heap block of exactly its size, `out` of exactly the capacity."""
    prog = C._make("emit_sanitize")
    files = []
    for which, (data, off, dec, seq, plan) in (("hand", hand), ("rnd", rnd)):
        n = off.size - 1
        full = C.ref_emit(data, off, dec, plan, C.TOPIC_IDS, C.IDENTS, seq=seq, term=0x0102030405060708, sess=-2)
        for c, case in enumerate(CASES):
            kw = _kw(case, n, full, seq)
            exp = C.ref_emit(data, off, dec, plan, C.TOPIC_IDS, C.IDENTS, **kw)
            path = tmp_path / f"{which}{c}.bin"
            _write_case(path, data, off, dec, plan, kw["seq"], kw.get("mask"), kw.get("flags", 0),
                        kw.get("session", True), kw["term"], kw["sess"], kw.get("cap"), exp)
            files.append(str(path))
    r = subprocess.run([prog] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(files)} cases ok" in r.stdout
