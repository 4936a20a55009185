"""Shared by test_commit_fallback_ref.py (CPU) and test_gpu_commit_fallback.py: the expected output
of sbe_emit_commit_offsets_ex with a fallback as a composition of things already trusted, the
batches both suites use, and the ctypes front end of tests/commitfallback/fallback_host_check.so.

The composition: autocommit_lib.ref_classify gives the plan; commitsend_lib.ref_emit gives every
Lite frame (the named tokens outside the table through four extra table entries with the default
identifier); the JSON text is restated here in a few lines (quote / text below, the quoting pinned
to the oracle's by test_commit_fallback_ref.py); the oracle's TopicMessage encoder in
SBE_ENC_PUBLISH_TOPIC mode, which has the same u16 wrap, builds the record from its five strings;
commitsend_lib.session_header goes in front.  Only the selection rules of include/sbecodec.h, the
1040-byte rule and the capacity rule are restated."""
import ctypes
import os
import struct
import subprocess

import numpy as np

import autocommit_lib as A
import commitsend_lib as C
import sbe_testlib as T

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "commitfallback")
NONE, EMITTED, HOST, E109, OVERFLOW, EMITTED_JSON, E100 = range(7)
LAST_ONLY = 1
KEYS = C.KEYS
REC_MAX = 1040
NAMES = {b"order_request_topic": 1, b"order_notification_topic": 2, b"orders": 3, b"order_status_request_topic": 4}
NOW, UUID0 = 1_700_000_000_123_456_789, 1_700_000_000_999_999_990
DEFAULT_IDENT = b"client-\xc3\xa9-0"

# the topic table of both suites: commitsend_lib's, whose entry 4 ("gamma") has id 0, with id 0
# for the fallback topic "default" (entry 0) as well
TOPICS = [b"default", b"alpha", b"beta", b"alpha", b"gamma", b'a"b', b""]
TOPIC_IDS = [0, 22, 33, 44, 0, 0x80000001, 77]
IDENTS = [b"client-7", b"sub-alpha", b"", b"dup", b'z"\x01z', b"x" * 17, b"e"]


def _make(target):
    subprocess.run(["make", "-s", "-C", DIR, target], check=True)
    return os.path.join(DIR, target)


def _cp(s, i):
    """jsoncpp utf8ToCodepoint: (code point, bytes used) of the sequence at s[i]."""
    b, left = s[i], len(s) - i
    if b < 0x80:
        return b, 1
    if b < 0xE0:
        if left < 2:
            return 0xFFFD, 1
        c = ((b & 0x1F) << 6) | (s[i + 1] & 0x3F)
        return (0xFFFD if c < 0x80 else c), 2
    if b < 0xF0:
        if left < 3:
            return 0xFFFD, 1
        c = ((b & 0x0F) << 12) | ((s[i + 1] & 0x3F) << 6) | (s[i + 2] & 0x3F)
        return (0xFFFD if 0xD800 <= c <= 0xDFFF or c < 0x800 else c), 3
    if b < 0xF8:
        if left < 4:
            return 0xFFFD, 1
        c = ((b & 0x07) << 18) | ((s[i + 1] & 0x3F) << 12) | ((s[i + 2] & 0x3F) << 6) | (s[i + 3] & 0x3F)
        return (0xFFFD if c < 0x10000 else c), 4
    return 0xFFFD, 1


_SHORT = {0x22: b'\\"', 0x5C: b"\\\\", 8: b"\\b", 12: b"\\f", 10: b"\\n", 13: b"\\r", 9: b"\\t"}


def quote(s: bytes) -> bytes:
    """valueToQuotedStringN(s, emitUTF8 = false)."""
    out, i = [b'"'], 0
    while i < len(s):
        c = s[i]
        if c in _SHORT:
            out.append(_SHORT[c])
            i += 1
        elif 0x20 <= c < 0x80:
            out.append(bytes([c]))
            i += 1
        else:
            cp, used = _cp(s, i)
            i += used
            if cp < 0x10000:
                out.append(b"\\u%04x" % cp)
            else:
                cp -= 0x10000
                out.append(b"\\u%04x\\u%04x" % (0xD800 + ((cp >> 10) & 0x3FF), 0xDC00 + (cp & 0x3FF)))
    out.append(b'"')
    return b"".join(out)


def text(topic, ident, mid, seq, ts) -> bytes:
    return (b'{"action":"COMMIT_OFFSET","messageIdentifier":' + quote(ident) + b',"message_id":' + quote(mid) +
            b',"sequence_number":%d,"timestamp_nanos":%d,"topic":' % (seq, ts) + quote(topic) + b"}")


def uuid(ident, clock) -> bytes:
    return b"commit_offset_" + ident + b"_%d" % clock


def json_fields(topic, ident, mid, seq, ts, clock):
    """The five strings of the record, or None where the reference throws [E100]."""
    u, t = uuid(ident, clock), text(topic, ident, mid, seq, ts)
    if 63 + (len(u) & 0xFFFF) + (len(t) & 0xFFFF) > REC_MAX:
        return None
    return [b"_subscriptions", b"COMMIT_OFFSET", u, t, b"{}"]


def encode_records(fields, now):
    """The oracle's TopicMessage encoder, publish_topic mode, over a list of five-string records."""
    if not fields:
        return []
    arena = np.frombuffer(b"".join(b"".join(f) for f in fields), np.uint8)
    L = np.array([[len(s) for s in f] for f in fields], np.uint32)
    out, off, st = T.oracle_encode(arena, L, np.full(len(fields), now, np.uint64), flags=T.ENC_PUBLISH_TOPIC,
                                   ts_default=now)
    assert (st == 0).all()
    return [out[int(off[r]): int(off[r + 1])] for r in range(len(fields))]


def ref_emit(data, rec_off, dec, plan, topics=TOPICS, topic_ids=TOPIC_IDS, idents=IDENTS, default_ident=DEFAULT_IDENT,
             now=NOW, uuid_ns=UUID0, seq=None, mask=None, flags=0, session=True, term=0, sess=0, cap=None):
    """Expected outputs of the call with a fallback: dict(out, out_off, status, emit_idx, totals)."""
    n, k = rec_off.size - 1, len(topic_ids)
    cm2, tidx2 = plan["cm"].copy(), plan["topic_idx"].copy()
    jrec = []  # (i, five strings or None)
    for i in range(n):
        if plan["cm"][i] != A.COMMIT or (mask is not None and not mask[i]):
            continue
        j = int(plan["topic_idx"][i])
        if j < k:
            if (flags & LAST_ONLY) and int(plan["last"][j]) != i:
                cm2[i] = A.NOT_PARSED
                continue
            if topic_ids[j] != 0:
                continue  # the Lite frame of commitsend_lib.ref_emit
            topic, ident = bytes(topics[j]), bytes(idents[j])
        elif j == A.UNKNOWN and plan["topic_kind"][i] == A.K_STR:
            b = int(rec_off[i]) + int(plan["topic_off"][i])
            topic, ident = bytes(data[b: b + int(plan["topic_len"][i])]), bytes(default_ident)
            if topic in NAMES:
                tidx2[i] = k + NAMES[topic] - 1
                continue
        else:
            continue  # stays SBE_CE_HOST
        cm2[i] = A.NOT_PARSED  # not ref_emit's business
        b = int(rec_off[i]) + int(dec["view_off"][i, 2])
        mid = bytes(data[b: b + int(dec["view_len"][i, 2])])
        has = seq is not None and dec["status"][i] == T.ST_TM and dec["flags"][i] & (T.FL_SEQ_KEY | T.FL_SEQ_ESC)
        jrec.append((i, json_fields(topic, ident, mid, int(seq[i]) if has else 0, int(dec["ts"][i]),
                                    (uuid_ns + i) % 2**64)))
    plan2 = dict(plan, cm=cm2, topic_idx=tidx2)
    lite = C.ref_emit(data, rec_off, dec, plan2, list(topic_ids) + [1, 2, 3, 4], list(idents) + [default_ident] * 4,
                      seq=seq, mask=mask, flags=0, session=session, term=term, sess=sess)
    status = lite["status"].copy()
    hdr = C.session_header(term, sess) if session else np.zeros(0, np.uint8)
    recs = encode_records([f for _, f in jrec if f is not None], now)
    frames, r = {}, 0
    for i, f in jrec:
        if f is None:
            status[i] = E100
        else:
            status[i] = EMITTED_JSON
            frames[i] = np.concatenate([hdr, recs[r]])
            r += 1
    for i in lite["emit_idx"]:
        i = int(i)
        frames[i] = lite["out"][int(lite["out_off"][i]): int(lite["out_off"][i + 1])]
    sizes = np.zeros(n, np.uint64)
    for i, f in frames.items():
        sizes[i] = f.size
    out_off = np.zeros(n + 1, np.uint64)
    out_off[1:] = np.cumsum(sizes)
    sel, parts = sorted(frames), []
    for i in sel:
        if cap is not None and int(out_off[i + 1]) > cap:
            status[i] = OVERFLOW
        else:
            parts.append(frames[i])
    out = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    totals = np.array([len(sel), int(out_off[n]), int((status == HOST).sum())], np.uint64)
    return dict(out=out, out_off=out_off, status=status, emit_idx=np.array(sel, np.uint64), totals=totals)


def host_arrays(data, rec_off, dec, plan, topics, topic_ids, idents, default_ident, seq, mask):
    """The input arrays of chk_emit_fb, in its argument order (None where absent)."""
    tarena, toff = topics if isinstance(topics, tuple) else A.topic_table(topics)
    iarena, ioff = idents if isinstance(idents, tuple) else A.topic_table(idents)
    c = np.ascontiguousarray
    return [c(data if data.size else np.zeros(1, np.uint8), np.uint8), c(rec_off, np.uint64), c(dec["status"]),
            c(dec["flags"]), c(dec["view_off"], np.uint32), c(dec["view_len"], np.uint32),
            None if seq is None else c(seq, np.uint64), c(dec["ts"], np.uint64), c(plan["cm"]), c(plan["topic_kind"]),
            c(plan["topic_off"], np.uint32), c(plan["topic_len"], np.uint32), c(plan["topic_idx"], np.uint32),
            c(plan["last"], np.uint64), np.asarray(topic_ids, np.uint32), iarena, c(ioff, np.uint32), tarena,
            c(toff, np.uint32)], np.frombuffer(bytes(default_ident), np.uint8), \
        None if mask is None else c(mask, np.uint8)


def chk_emit(data, rec_off, dec, plan, topics=TOPICS, topic_ids=TOPIC_IDS, idents=IDENTS, default_ident=DEFAULT_IDENT,
             now=NOW, uuid_ns=UUID0, seq=None, mask=None, flags=0, session=True, term=0, sess=0, cap=None):
    """The device functions compiled for the host (fallback_host_check.cpp), driven as the launches
    drive them; same result layout as ref_emit."""
    lib = ctypes.CDLL(_make("fallback_host_check.so"))
    n = rec_off.size - 1
    arrs, dident, maskv = host_arrays(data, rec_off, dec, plan, topics, topic_ids, idents, default_ident, seq, mask)
    bound = int(rec_off[n] - rec_off[0]) + n * (56 + 4096 + 1072) + 16
    capv = bound if cap is None else cap
    out = np.full(bound + 64, 0xEE, np.uint8)
    m = max(n, 1)
    res = dict(out_off=np.zeros(n + 1, np.uint64), status=np.zeros(m, np.uint8), emit_idx=np.zeros(m, np.uint64),
               totals=np.zeros(3, np.uint64))
    p, u32, u64, i64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64

    def ptr(a):
        return None if a is None else a.ctypes.data_as(p)

    dbuf = dident if dident.size else np.zeros(1, np.uint8)
    f = lib.chk_emit_fb
    f.restype = ctypes.c_int
    f.argtypes = [p, p, u64] + [p] * 17 + [u32, p, u32, u64, u64, p, u32, ctypes.c_int, i64, i64, p, u64, p, p, p, p]
    rc = f(ptr(arrs[0]), ptr(arrs[1]), n, *(ptr(a) for a in arrs[2:]), len(topic_ids), ptr(dbuf), dident.size,
           now, uuid_ns, ptr(maskv), flags, 1 if session else 0, term, sess, ptr(out), capv,
           *(ptr(res[key]) for key in KEYS))
    if rc == -1:
        raise ValueError("SBE_EINVAL")
    assert rc == 0, rc
    end = 0
    fit = np.nonzero((res["status"][:n] == EMITTED) | (res["status"][:n] == EMITTED_JSON))[0]
    if fit.size:
        end = int(res["out_off"][fit[-1] + 1])
    assert (out[end:] == 0xEE).all(), "bytes past the last frame that fits were written"
    res["out"] = out[:end]
    res["status"] = res["status"][:n]
    res["emit_idx"] = res["emit_idx"][: int(res["totals"][0])]
    return res


same = C.same


def frame(res, i):
    return bytes(res["out"][int(res["out_off"][i]): int(res["out_off"][i + 1])])


# ------------------------------------------------------------------------------------------
# the hand table: (message_type, message_id, payload, headers, ts) -> status, one line per rule
# ------------------------------------------------------------------------------------------
P, PSEQ = C.P, C.PSEQ
ESC_ID = b'q"b\\s\x08\x0c\n\r\t\x00\x01\x1f\x7f\xc3\xa9\xe2\x82\xac\xf0\x9f\x98\x80\xff\xc3'
HAND = [
    ((b"X", b"m-gamma", P, b'{"topic":"gamma"}', 1_001), EMITTED_JSON),        # an id-0 table entry (its identifier escapes)
    ((b"CREATE_ORDER", b"m-fallback", P, b"{}", 1_002), EMITTED_JSON),          # the fallback topic, id 0
    ((b"X", b"m-delta", PSEQ, b'{"topic":"delta"}', 1_003), EMITTED_JSON),      # unknown plain topic, a flagged sequence
    ((b"X", b"m-orders", P, b'{"topic":"orders"}', 1_004), EMITTED),            # unknown, one of the four names: Lite, id 3
    ((b"X", b"m-ort", PSEQ, b'{"topic":"order_request_topic"}', 1_005), EMITTED),
    ((b"X", b"m-esc", P, b'{"topic":"delt\\u0061"}', 1_006), HOST),             # unknown escaped topic
    ((b"X", b"m-12", P, b'{"topic":12}', 1_007), HOST),                         # number topic
    ((b"X", ESC_ID, P, b'{"topic":"t\x01\xc3\xa9\xf0\x9f\x98\x80/\x7f\xfe"}', 1_008), EMITTED_JSON),  # every escape class
    ((b"X", b"m-alpha", PSEQ, b'{"topic":"alpha"}', 1_009), EMITTED),           # a table entry with an id
    ((b"X", b"m-neg", P, b'{"topic":"delta"}', 2**64 - 5), EMITTED_JSON),       # negative ts: printed as u64
    ((b"X", b"m-poison", P, b'{"topic":"gamma"}', 0), EMITTED_JSON),            # unflagged: sequence 0 over a poisoned seq
    ((b"SUBSCRIBE", b"m1", P, b"{}", 5), NONE),
    ((b"X", b"", P, b'{"topic":"gamma"}', 5), NONE),
    ((b"X", b"i" * 65535, P, b'{"topic":"orders"}', 5), E109),                  # the Lite rule for a named token
    ((b"X", b"i" * 2000, P, b'{"topic":"gamma"}', 5), E100),
    ((b"X", b"m-empty", P, b'{"topic":""}', 6), EMITTED),
    ((b"X", b"m-orderz", P, b'{"topic":"orderz"}', 7), EMITTED_JSON),           # a near miss of a name
    ((b"X", b"m-last", P, b'{"topic":"gamma"}', 8), EMITTED_JSON),
]


def hand_records():
    recs = [T.tm_wire([b"orders", ty, mid, pl, hd], ts) for (ty, mid, pl, hd, ts), _ in HAND]
    return recs + [T.ack_wire(b"id1", b"orders", b"c", 5), T.session_event(1, 9, 7, 1, 0, b"detail"), b"\x01"]


def hand_status():
    return np.array([s for _, s in HAND] + [NONE, NONE, NONE], np.uint8)


def fill_id(fixed_text_len, want_text_len):
    """A plain id that brings a text whose other parts take fixed_text_len bytes to want_text_len."""
    return b"f" * (want_text_len - fixed_text_len)


def skeleton_len(topic, ident, seq, ts):
    """Text bytes apart from the id's own characters (an id of plain bytes adds one each)."""
    return len(text(topic, ident, b"", seq, ts))


RANDOM_SEED, RANDOM_N = 0xCF01, 3000


def random_records(n=RANDOM_N, seed=RANDOM_SEED):
    """autocommit_lib's random batch (id-0, unknown and host-resolved topics among the rest) with an
    id over the Lite limit on a named token, and a JSON record over the 1040-byte bound."""
    recs = A.random_records(n, seed)
    recs[n // 2] = T.tm_wire([b"orders", b"X", b"k" * 65535, P, b'{"topic":"beta"}'], 7)
    recs[n // 2 + 1] = T.tm_wire([b"orders", b"X", b"k" * 1500, P, b'{"topic":"gamma"}'], 8)
    return recs


def write_case(path, data, off, dec, plan, exp, seq=None, mask=None, flags=0, session=True, term=0, sess=0, cap=None,
               topics=TOPICS, topic_ids=TOPIC_IDS, idents=IDENTS, default_ident=DEFAULT_IDENT, now=NOW, uuid_ns=UUID0):
    """A case file of tests/commitfallback/fallback_sanitize_main.cpp."""
    n, k = off.size - 1, len(topic_ids)
    arrs, dident, maskv = host_arrays(data, off, dec, plan, topics, topic_ids, idents, default_ident, seq, mask)
    arrs[0] = np.ascontiguousarray(data, np.uint8)
    cap = int(exp["out_off"][-1]) if cap is None else cap
    head = np.array([0x3130424643544d43, n, k, data.size, flags, int(session), term % 2**64, sess % 2**64, cap,
                     seq is not None, mask is not None, exp["out"].size, dident.size, now, uuid_ns], np.uint64)
    parts = [head] + [a for a in arrs if a is not None] + [dident] + ([] if maskv is None else [maskv])
    parts += [exp["out_off"], exp["status"], exp["totals"], exp["emit_idx"], exp["out"]]
    with open(path, "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p).tobytes())


def spelled_out(term, sess, now, ident, clock, txt):
    """One frame written out byte for byte (the CPU suite's anchor)."""
    u = uuid(ident, clock)
    return (struct.pack("<4Hqqq", 24, 1, 111, 8, term, sess, 0) + struct.pack("<4HQQ", 16, 1, 1, 1, now, 0) +
            struct.pack("<H", 14) + b"_subscriptions" + struct.pack("<H", 13) + b"COMMIT_OFFSET" +
            struct.pack("<H", len(u)) + u + struct.pack("<H", len(txt)) + txt + struct.pack("<H", 2) + b"{}")
