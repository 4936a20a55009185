"""Shared by test_commit_emit_ref.py (CPU) and test_gpu_commit_emit.py: the expected output of
sbe_emit_commit_offsets as a composition of things already trusted, the batches both suites use,
and the ctypes front end of tests/commitsend/emit_host_check.so (the device sizing and writing
functions of csrc/commit_emit.hpp compiled for the host).

The composition: autocommit_lib.ref_classify gives the plan; the oracle's orc_encode_lite_batch
(template 301) encodes the selected records' uuid views and identifiers; every record is prefixed
with the 32 session header bytes orc_encode_session_batch produces for the same ids.  Only the
selection (the status table of include/sbecodec.h) and the capacity rule are restated here."""
import ctypes
import os
import subprocess

import numpy as np

import autocommit_lib as A
import sbe_testlib as T

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "commitsend")
NONE, EMITTED, HOST, E109, OVERFLOW = range(5)
LAST_ONLY = 1
KEYS = ("out_off", "status", "emit_idx", "totals")
POISON = 0xDEADBEEFCAFEF00D

# the topic table of both suites: a duplicate topic (entry 3 never matches) and an entry with id 0
TOPICS = [b"orders", b"alpha", b"beta", b"alpha", b"gamma", b'a"b', b""]
TOPIC_IDS = [11, 22, 33, 44, 0, 0x80000001, 77]
IDENTS = [b"client-7", b"sub-alpha", b"", b"dup", b"zz", b"x" * 17, b"e"]


def _make(target):
    subprocess.run(["make", "-s", "-C", DIR, target], check=True)
    return os.path.join(DIR, target)


def batch(recs, lead=0):
    """(data, rec_off, dec, seq): recs packed with `lead` filler bytes in front (rec_off[0] = lead), the
    oracle's parse-mode descriptors and its sequence numbers with a poison in every unwritten slot."""
    data, off = T.pack_records(recs)
    if lead:
        data = np.concatenate([np.full(lead, 0xA5, np.uint8), data])
        off = off + np.uint64(lead)
    dec = T.oracle_decode(data, off, T.DEC_PARSE)
    seq = T.oracle_seq_batch(data, off, dec).copy()
    flagged = (dec["status"] == T.ST_TM) & ((dec["flags"] & (T.FL_SEQ_KEY | T.FL_SEQ_ESC)) != 0)
    seq[~flagged] = POISON
    return data, off, dec, seq


def session_header(term, sess):
    """The 32 bytes orc_encode_session_batch puts in front of a record for these ids."""
    out, _, _ = T.oracle_encode_session(np.zeros(1, np.uint8), np.zeros((1, 5), np.uint32), np.ones(1, np.uint64),
                                        term, sess)
    return out[:32].copy()


def ref_emit(data, rec_off, dec, plan, topic_ids, idents, seq=None, mask=None, flags=0, session=True, term=0,
             sess=0, cap=None):
    """Expected outputs: dict(out, out_off, status, emit_idx, totals); out holds the frames that fit
    cap (None: all of them)."""
    n = rec_off.size - 1
    k = len(topic_ids)
    status = np.zeros(n, np.uint8)
    sel, ids, tid, sq = [], [], [], []
    for i in range(n):
        if plan["cm"][i] != A.COMMIT or (mask is not None and not mask[i]):
            continue
        j = int(plan["topic_idx"][i])
        if j >= k or topic_ids[j] == 0:
            status[i] = HOST
            continue
        if (flags & LAST_ONLY) and int(plan["last"][j]) != i:
            continue
        ln = int(dec["view_len"][i, 2])
        if ln > 65534:
            status[i] = E109
            continue
        status[i] = EMITTED
        b = int(rec_off[i]) + int(dec["view_off"][i, 2])
        sel.append(i)
        ids.append((bytes(data[b: b + ln]), bytes(idents[j])))
        tid.append(topic_ids[j])
        has = seq is not None and dec["status"][i] == T.ST_TM and dec["flags"][i] & (T.FL_SEQ_KEY | T.FL_SEQ_ESC)
        sq.append(int(seq[i]) if has else 0)
    m = len(sel)
    arena = np.frombuffer(b"".join(a + b for a, b in ids), np.uint8)
    lens = np.array([[len(a), len(b)] for a, b in ids], np.uint32).reshape(m, 2)
    lite, loff, lst = T.oracle_encode_lite(301, arena, lens, np.array(tid, np.uint32), np.array(sq, np.uint64))
    assert (lst == 0).all()
    hdr = session_header(term, sess) if session else np.zeros(0, np.uint8)
    sizes = np.zeros(n, np.uint64)
    sizes[sel] = np.diff(loff) + np.uint64(hdr.size)
    out_off = np.zeros(n + 1, np.uint64)
    out_off[1:] = np.cumsum(sizes)
    parts = []
    for r, i in enumerate(sel):
        if cap is not None and int(out_off[i + 1]) > cap:
            status[i] = OVERFLOW
            continue
        parts += [hdr, lite[int(loff[r]): int(loff[r + 1])]]
    out = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    totals = np.array([m, int(out_off[n]), int((status == HOST).sum())], np.uint64)
    return dict(out=out, out_off=out_off, status=status, emit_idx=np.array(sel, np.uint64), totals=totals)


def ident_table(idents):
    return A.topic_table(idents)


def chk_emit(data, rec_off, dec, plan, topic_ids, idents, seq=None, mask=None, flags=0, session=True, term=0,
             sess=0, cap=None):
    """The device functions compiled for the host (emit_host_check.cpp), driven as the launches
    drive them; same result layout as ref_emit.  idents: a list or an (arena, off) pair."""
    lib = ctypes.CDLL(_make("emit_host_check.so"))
    n = rec_off.size - 1
    arena, ioff = idents if isinstance(idents, tuple) else ident_table(idents)
    bound = int(rec_off[n] - rec_off[0]) + n * (56 + 4096) + 16
    capv = bound if cap is None else cap
    out = np.full(bound + 64, 0xEE, np.uint8)
    m = max(n, 1)
    res = dict(out_off=np.zeros(n + 1, np.uint64), status=np.zeros(m, np.uint8), emit_idx=np.zeros(m, np.uint64),
               totals=np.zeros(3, np.uint64))
    p = ctypes.c_void_p

    def ptr(a, t=None):
        return None if a is None else np.ascontiguousarray(a, t).ctypes.data_as(p)

    keep = [np.ascontiguousarray(data if data.size else np.zeros(1, np.uint8), np.uint8),
            np.ascontiguousarray(rec_off, np.uint64), np.ascontiguousarray(dec["status"]),
            np.ascontiguousarray(dec["flags"]), np.ascontiguousarray(dec["view_off"], np.uint32),
            np.ascontiguousarray(dec["view_len"], np.uint32),
            None if seq is None else np.ascontiguousarray(seq, np.uint64), np.ascontiguousarray(plan["cm"]),
            np.ascontiguousarray(plan["topic_idx"], np.uint32), np.ascontiguousarray(plan["last"], np.uint64),
            np.asarray(topic_ids, np.uint32), arena, np.ascontiguousarray(ioff, np.uint32)]
    f = lib.chk_emit
    f.restype = ctypes.c_int
    f.argtypes = [p, p, ctypes.c_uint64] + [p] * 11 + [ctypes.c_uint32, p, ctypes.c_uint32, ctypes.c_int,
                                                      ctypes.c_int64, ctypes.c_int64, p, ctypes.c_uint64, p, p, p, p]
    rc = f(ptr(keep[0]), ptr(keep[1]), n, *(ptr(a) for a in keep[2:]), len(topic_ids),
           ptr(None if mask is None else np.ascontiguousarray(mask, np.uint8)), flags, 1 if session else 0, term,
           sess, ptr(out), capv, *(ptr(res[key]) for key in KEYS))
    if rc == -1:
        raise ValueError("SBE_EINVAL")
    assert rc == 0, rc
    end = 0
    fit = np.nonzero(res["status"][:n] == EMITTED)[0]
    if fit.size:
        end = int(res["out_off"][fit[-1] + 1])
    assert (out[end:] == 0xEE).all(), "bytes past the last frame that fits were written"
    res["out"] = out[:end]
    res["status"] = res["status"][:n]
    res["emit_idx"] = res["emit_idx"][: int(res["totals"][0])]
    return res


def same(got, exp, what=""):
    """Byte for byte and element for element."""
    for key in KEYS:
        g, e = np.asarray(got[key]), np.asarray(exp[key])
        assert g.shape == e.shape, (what, key, g.shape, e.shape)
        bad = np.nonzero(g != e)[0]
        assert bad.size == 0, (what, key, bad[:5], g[bad[:5]], e[bad[:5]])
    g, e = np.asarray(got["out"]), np.asarray(exp["out"])
    assert g.size >= e.size, (what, "out", g.size, e.size)
    bad = np.nonzero(g[: e.size] != e)[0]
    assert bad.size == 0, (what, "out", bad[:5])


# ------------------------------------------------------------------------------------------
# the hand table: (message_type, message_id, payload, headers) -> status
# ------------------------------------------------------------------------------------------
P = b'{"x":1}'
PSEQ = b'{"_sequence_number": 123456789012, "x":1}'
HAND = [
    ((b"CREATE_ORDER", b"m-fallback", P, b"{}"), EMITTED),                   # entry 0
    ((b"X", b"m-alpha", PSEQ, b'{"topic":"alpha"}'), EMITTED),               # entry 1, a sequence number
    ((b"X", b"m-beta", P, b'{"topic":"beta"}'), EMITTED),                    # entry 2, empty identifier
    ((b"X", b"m-gamma", P, b'{"topic":"gamma"}'), HOST),                     # entry 4 has id 0
    ((b"X", b"m-delta", P, b'{"topic":"delta"}'), HOST),                     # SBE_TOPIC_UNKNOWN
    ((b"X", b"m-12", P, b'{"topic":12}'), HOST),                             # SBE_TOPIC_HOST
    ((b"X", b"m-esc", P, b'{"topic":"\\u0061lpha"}'), EMITTED),              # an escaped spelling of entry 1
    ((b"X", b"m-quote", PSEQ, b'{"topic":"a\\"b"}'), EMITTED),               # entry 5, topic id with the top bit
    ((b"X", b"m-empty", P, b'{"topic":""}'), EMITTED),                       # entry 6
    ((b"SUBSCRIBE", b"m1", P, b"{}"), NONE),
    ((b"X", b"ack_1", P, b"{}"), NONE),
    ((b"X", b"", P, b'{"topic":"alpha"}'), NONE),
    ((b"X", b"m1", b"", b"{}"), NONE),
    ((b"X", b"i" * 65535, P, b'{"topic":"alpha"}'), E109),
    ((b"X", b"j" * 65534, P, b'{"topic":"alpha"}'), EMITTED),
    ((b"X", b"m-last", P, b'{"topic":"beta"}'), EMITTED),
]


def hand_records():
    recs = [T.tm_wire([b"orders", ty, mid, pl, hd], 1_000 + i) for i, ((ty, mid, pl, hd), _) in enumerate(HAND)]
    return recs + [T.ack_wire(b"id1", b"orders", b"c", 5), T.session_event(1, 9, 7, 1, 0, b"detail"), b"\x01"]


def hand_status():
    return np.array([s for _, s in HAND] + [NONE, NONE, NONE], np.uint8)


RANDOM_SEED, RANDOM_N = 0xCE01, 3000


def random_records(n=RANDOM_N, seed=RANDOM_SEED):
    """autocommit_lib's random batch (every commit code, every topic source) with one id of 65535
    bytes in the middle."""
    recs = A.random_records(n, seed)
    recs[n // 2] = T.tm_wire([b"orders", b"X", b"k" * 65535, P, b'{"topic":"beta"}'], 7)
    return recs
