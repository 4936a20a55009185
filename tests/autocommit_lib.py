"""Shared by test_autocommit_ref.py (CPU) and test_gpu_autocommit.py: the hand table, the seeded
random batch and the ctypes front ends of tests/autocommit (the reference restatement
commit_ref.so and the host build of the device classifier commit_host_check.so)."""
import ctypes
import os
import random
import subprocess

import numpy as np

import sbe_testlib as T

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "autocommit")

COMMIT, NOT_PARSED, SKIP_TYPE, SKIP_ACK_ID, SKIP_TOPIC, SKIP_CONTROL, SKIP_EMPTY, NO_ID = range(8)
NONE, HEADERS, PAYLOAD, PAYLOAD_MESSAGE, FALLBACK = range(5)
K_NONE, K_STR, K_ESC, K_NUM, K_TRUE, K_FALSE, K_NULL = range(7)
UNKNOWN, HOST = 0xFFFFFFFF, 0xFFFFFFFE
TABLE_BYTES = 4096
KEYS = ("cm", "topic_src", "topic_kind", "topic_off", "topic_len", "topic_idx", "last", "count")

_libs = {}


def _lib(name):
    if name not in _libs:
        subprocess.run(["make", "-s", "-C", DIR, name + ".so"], check=True)
        _libs[name] = ctypes.CDLL(os.path.join(DIR, name + ".so"))
    return _libs[name]


def ref_seq(doc: bytes) -> int:
    f = _lib("commit_ref").cref_seq
    f.restype = ctypes.c_uint64
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    buf = np.frombuffer(doc, np.uint8) if doc else np.zeros(1, np.uint8)
    return int(f(buf.ctypes.data_as(ctypes.c_void_p), len(doc)))


def topic_table(topics):
    off = np.zeros(len(topics) + 1, np.uint32)
    off[1:] = np.cumsum([len(t) for t in topics])
    arena = np.zeros(TABLE_BYTES, np.uint8)
    arena[: int(off[-1])] = np.frombuffer(b"".join(topics), np.uint8)
    return arena, off


def _classify(lib, fn, data, rec_off, dec, topics):
    arena, toff = topics if isinstance(topics, tuple) else topic_table(topics)
    k = toff.size - 1
    data = np.ascontiguousarray(data, np.uint8)
    rec_off = np.ascontiguousarray(rec_off, np.uint64)
    n = rec_off.size - 1
    m = max(n, 1)
    out = dict(cm=np.zeros(m, np.uint8), topic_src=np.zeros(m, np.uint8), topic_kind=np.zeros(m, np.uint8),
               topic_off=np.zeros(m, np.uint32), topic_len=np.zeros(m, np.uint32), topic_idx=np.zeros(m, np.uint32),
               last=np.zeros(k, np.uint64), count=np.zeros(k + 2, np.uint64))
    ins = [data if data.size else np.zeros(1, np.uint8), rec_off] + \
          [np.ascontiguousarray(dec[f]) for f in ("status", "flags", "view_off", "view_len")] + [arena, toff]
    f = getattr(_lib(lib), fn)
    f.restype = None
    p = ctypes.c_void_p
    f.argtypes = [p, p, ctypes.c_uint64, p, p, p, p, p, p, ctypes.c_uint32] + [p] * 8
    ptr = [a.ctypes.data_as(p) for a in ins]
    f(ptr[0], ptr[1], n, *ptr[2:8], k, *(out[key].ctypes.data_as(p) for key in KEYS))
    for key in KEYS[:6]:
        out[key] = out[key][:n]
    return out


def ref_classify(data, rec_off, dec, topics):
    """The restatement (commit_ref.cpp) on host arrays: the expected outputs of sbe_classify_commits."""
    return _classify("commit_ref", "cref_classify", data, rec_off, dec, topics)


def chk_classify(data, rec_off, dec, topics):
    """The device classifier compiled for the host (commit_host_check.cpp)."""
    return _classify("commit_host_check", "chk_classify", data, rec_off, dec, topics)


# ------------------------------------------------------------------------------------------
# the hand table: (message_type, message_id, payload, headers) -> (cm, src, kind, token, idx)
# token: the bytes topic_off / topic_len must select in the record (None: both 0)
# ------------------------------------------------------------------------------------------
TOPICS = [b"orders", b"alpha", b"beta", b"alpha", b"_control", b'a"b', b""]
P = b'{"x":1}'
_DEEP_OK = b'{"topic":"alpha","a":' + b"[" * 999 + b"]" * 999 + b"}"
_DEEP = b'{"topic":"alpha","a":' + b"[" * 1000 + b"]" * 1000 + b"}"
FB = (FALLBACK, K_NONE, None)
HAND = [
    # the clauses, in order
    ((b"CREATE_ORDER", b"m1", P, b"{}"), (COMMIT, *FB, 0)),
    ((b"acknowledgment", b"m1", P, b"{}"), (SKIP_TYPE, NONE, K_NONE, None, UNKNOWN)),
    ((b"acknowledgment_legacy", b"m1", P, b"{}"), (SKIP_TYPE, NONE, K_NONE, None, UNKNOWN)),
    ((b"Acknowledgment", b"m1", P, b"{}"), (SKIP_TYPE, NONE, K_NONE, None, UNKNOWN)),
    ((b"Acknowledgment_legacy", b"m1", P, b"{}"), (SKIP_TYPE, NONE, K_NONE, None, UNKNOWN)),
    ((b"COMMIT_RESPONSE", b"m1", P, b"{}"), (SKIP_TYPE, NONE, K_NONE, None, UNKNOWN)),
    ((b"SUBSCRIBE", b"ack_1", P, b'{"topic":"_ack"}'), (SKIP_TYPE, NONE, K_NONE, None, UNKNOWN)),
    ((b"ACKNOWLEDGMENT", b"m1", P, b"{}"), (COMMIT, *FB, 0)),
    ((b"acknowledgment_legacx", b"m1", P, b"{}"), (COMMIT, *FB, 0)),
    ((b"SUBSCRIBED", b"m1", P, b"{}"), (COMMIT, *FB, 0)),
    ((b"", b"m1", P, b"{}"), (COMMIT, *FB, 0)),
    ((b"X", b"ack_1", P, b'{"topic":"alpha"}'), (SKIP_ACK_ID, NONE, K_NONE, None, UNKNOWN)),
    ((b"X", b"ack_", b"", b""), (SKIP_ACK_ID, NONE, K_NONE, None, UNKNOWN)),
    ((b"X", b"ack", P, b"{}"), (COMMIT, *FB, 0)),
    ((b"X", b"xack_1", P, b"{}"), (COMMIT, *FB, 0)),
    ((b"X", b"m1", P, b'{"topic":"_ack"}'), (SKIP_TOPIC, HEADERS, K_STR, b"_ack", UNKNOWN)),
    ((b"X", b"m1", b'{"topic":"_subscriptions"}', b""), (SKIP_TOPIC, PAYLOAD, K_STR, b"_subscriptions", UNKNOWN)),
    ((b"X", b"m1", b'{"message":{"topic":"_ack"}}', b"{}"), (SKIP_TOPIC, PAYLOAD_MESSAGE, K_STR, b"_ack", UNKNOWN)),
    ((b"X", b"m1", P, b'{"topic":"_control"}'), (SKIP_CONTROL, HEADERS, K_STR, b"_control", UNKNOWN)),
    ((b"X", b"", b"", b'{"topic":"_control"}'), (SKIP_CONTROL, HEADERS, K_STR, b"_control", UNKNOWN)),
    ((b"REPLAY_COMPLETE", b"m1", P, b'{"topic":"_control"}'), (COMMIT, HEADERS, K_STR, b"_control", 4)),
    ((b"REPLAY_COMPLETE", b"m1", b"", b'{"topic":"_control"}'), (COMMIT, HEADERS, K_STR, b"_control", 4)),
    ((b"REPLAY_COMPLETE", b"", b"", b'{"topic":"_control"}'), (NO_ID, HEADERS, K_STR, b"_control", UNKNOWN)),
    ((b"X", b"m1", b'{"k":"REPLAY_COMPLETE"}', b'{"topic":"_control"}'), (COMMIT, HEADERS, K_STR, b"_control", 4)),
    ((b"X", b"m1", b"xxREPLAY_COMPLETE", b'{"topic":"_control"}'), (COMMIT, HEADERS, K_STR, b"_control", 4)),
    ((b"X", b"m1", b"REPLAY_COMPLET", b'{"topic":"_control"}'), (SKIP_CONTROL, HEADERS, K_STR, b"_control", UNKNOWN)),
    ((b"REPLAY_COMPLETE", b"m1", b"", b"{}"), (SKIP_EMPTY, *FB, UNKNOWN)),
    ((b"X", b"m1", b"", b"{}"), (SKIP_EMPTY, *FB, UNKNOWN)),
    ((b"X", b"", b"", b""), (SKIP_EMPTY, *FB, UNKNOWN)),
    ((b"X", b"", P, b"{}"), (NO_ID, *FB, UNKNOWN)),
    ((b"X", b"", P, b'{"topic":"alpha"}'), (NO_ID, HEADERS, K_STR, b"alpha", UNKNOWN)),
    # extraction branches
    ((b"X", b"m1", P, b'{"topic":"alpha"}'), (COMMIT, HEADERS, K_STR, b"alpha", 1)),
    ((b"X", b"m1", b"", b'{"topic":"alpha"}'), (SKIP_EMPTY, HEADERS, K_STR, b"alpha", UNKNOWN)),
    ((b"X", b"m1", b'{"topic":"beta"}', b""), (COMMIT, PAYLOAD, K_STR, b"beta", 2)),
    ((b"X", b"m1", b'{"topic":"beta"}', b'{"a":1}'), (COMMIT, PAYLOAD, K_STR, b"beta", 2)),
    ((b"X", b"m1", b'{"topic":"beta"}', b'{"topic":"alpha"}'), (COMMIT, HEADERS, K_STR, b"alpha", 1)),
    ((b"X", b"m1", b'{"message":{"topic":"beta"}}', b""), (COMMIT, PAYLOAD_MESSAGE, K_STR, b"beta", 2)),
    ((b"X", b"m1", b'{"topic":"alpha","message":{"topic":"beta"}}', b""), (COMMIT, PAYLOAD, K_STR, b"alpha", 1)),
    ((b"X", b"m1", b'{"message":{"topic":"beta"},"topic":"alpha"}', b""), (COMMIT, PAYLOAD, K_STR, b"alpha", 1)),
    ((b"X", b"m1", b'{"message":{"message":{"topic":"beta"}}}', b""), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'{"a":{"topic":"beta"}}', b'{"a":{"topic":"alpha"}}'), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'{"message":{"a":{"topic":"beta"}}}', b'[{"topic":"alpha"}]'), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'{"x":"topic"}', b'{"topic_":"alpha"}'), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'{"message":{"topic":"beta"}}', b'{"message":{"topic":"alpha"}}'),
     (COMMIT, PAYLOAD_MESSAGE, K_STR, b"beta", 2)),
    # container-valued topic in each of the three places
    ((b"X", b"m1", b'{"topic":"beta"}', b'{"topic":[1]}'), (COMMIT, PAYLOAD, K_STR, b"beta", 2)),
    ((b"X", b"m1", P, b'{"topic":{"topic":"alpha"}}'), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'{"topic":{},"message":{"topic":"beta"}}', b""), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'{"message":{"topic":["beta"]}}', b""), (COMMIT, *FB, 0)),
    # roots and "message" values
    ((b"X", b"m1", b'{"topic":"beta"}', b"null"), (COMMIT, PAYLOAD, K_STR, b"beta", 2)),
    ((b"X", b"m1", b"null", b'"topic"'), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'[{"topic":"beta"}]', b""), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'"topic"', b"5"), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'{"message":"topic"}', b""), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'{"message":null,"a":"topic"}', b""), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'{"message":[{"topic":"beta"}]}', b""), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'{"message":{}, "a":"topic"}', b""), (COMMIT, *FB, 0)),
    # duplicate keys: the last one wins
    ((b"X", b"m1", P, b'{"topic":"alpha","topic":"beta"}'), (COMMIT, HEADERS, K_STR, b"beta", 2)),
    ((b"X", b"m1", b'{"topic":"beta"}', b'{"topic":"alpha","topic":[]}'), (COMMIT, PAYLOAD, K_STR, b"beta", 2)),
    ((b"X", b"m1", b'{"topic":[],"topic":"beta"}', b""), (COMMIT, PAYLOAD, K_STR, b"beta", 2)),
    ((b"X", b"m1", b'{"message":{"topic":"alpha"},"message":1}', b""), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'{"message":1,"message":{"topic":"alpha"}}', b""), (COMMIT, PAYLOAD_MESSAGE, K_STR, b"alpha", 1)),
    ((b"X", b"m1", b'{"message":{"topic":"alpha"},"message":{"a":1}}', b""), (COMMIT, *FB, 0)),
    ((b"X", b"m1", b'{"message":{"topic":"alpha","topic":"beta"}}', b""), (COMMIT, PAYLOAD_MESSAGE, K_STR, b"beta", 2)),
    # escapes
    ((b"X", b"m1", P, b'{"t\\u006fpic":"alpha"}'), (COMMIT, HEADERS, K_STR, b"alpha", 1)),
    ((b"X", b"m1", b'{"m\\u0065ssage":{"\\u0074opic":"beta"}}', b""), (COMMIT, PAYLOAD_MESSAGE, K_STR, b"beta", 2)),
    ((b"X", b"m1", P, b'{"topic":"_c\\u006fntrol"}'), (SKIP_CONTROL, HEADERS, K_ESC, b"_c\\u006fntrol", UNKNOWN)),
    ((b"X", b"m1", P, b'{"topic":"\\u005fack"}'), (SKIP_TOPIC, HEADERS, K_ESC, b"\\u005fack", UNKNOWN)),
    ((b"X", b"m1", P, b'{"topic":"\\u0061lpha"}'), (COMMIT, HEADERS, K_ESC, b"\\u0061lpha", 1)),
    ((b"X", b"m1", P, b'{"topic":"a\\"b"}'), (COMMIT, HEADERS, K_ESC, b'a\\"b', 5)),
    ((b"X", b"m1", P, b'{"topic":"al\\u0000pha"}'), (COMMIT, HEADERS, K_ESC, b"al\\u0000pha", UNKNOWN)),
    ((b"X", b"m1", P, b'{"topic":"alpha\\q"}'), (COMMIT, *FB, 0)),
    ((b"X", b"m1", P, b'{"topic\\u0000":"alpha"}'), (COMMIT, *FB, 0)),
    ((b"X", b"m1", P, b'{"a":"\\\\","b":2}'), (COMMIT, *FB, 0)),
    # jsoncpp-only syntax
    ((b"X", b"m1", P, b'/*c*/{"topic":"alpha"//x\n}'), (COMMIT, HEADERS, K_STR, b"alpha", 1)),
    ((b"X", b"m1", P, b'{"topic":"alpha",}'), (COMMIT, HEADERS, K_STR, b"alpha", 1)),
    ((b"X", b"m1", P, b'\xef\xbb\xbf{"topic":"alpha"}'), (COMMIT, HEADERS, K_STR, b"alpha", 1)),
    ((b"X", b"m1", P, b'{"topic":"alpha"} trailing {'), (COMMIT, HEADERS, K_STR, b"alpha", 1)),
    ((b"X", b"m1", P, b'{"topic":"alpha"}\x00{'), (COMMIT, HEADERS, K_STR, b"alpha", 1)),
    ((b"X", b"m1", P, b'{"topic":\x00"alpha"}'), (COMMIT, *FB, 0)),
    ((b"X", b"m1", P, b'{"topic":"alpha'), (COMMIT, *FB, 0)),
    ((b"X", b"m1", P, b'{"topic":"alpha","x":}'), (COMMIT, *FB, 0)),
    ((b"X", b"m1", P, b'{"topic":"alpha","x":1e}'), (COMMIT, *FB, 0)),
    ((b"X", b"m1", P, b"{'topic':'alpha'}"), (COMMIT, *FB, 0)),
    ((b"X", b"m1", P, b'{"topic":"alpha",,}'), (COMMIT, *FB, 0)),
    ((b"X", b"m1", P, _DEEP_OK), (COMMIT, HEADERS, K_STR, b"alpha", 1)),
    ((b"X", b"m1", b'{"topic":"beta"}', _DEEP), (COMMIT, PAYLOAD, K_STR, b"beta", 2)),
    # non-string topics
    ((b"X", b"m1", P, b'{"topic":12}'), (COMMIT, HEADERS, K_NUM, b"12", HOST)),
    ((b"X", b"m1", P, b'{"topic": -1.5e3 }'), (COMMIT, HEADERS, K_NUM, b"-1.5e3", HOST)),
    ((b"X", b"m1", b'{"topic":true}', b""), (COMMIT, PAYLOAD, K_TRUE, b"true", HOST)),
    ((b"X", b"m1", b'{"message":{"topic":false}}', b""), (COMMIT, PAYLOAD_MESSAGE, K_FALSE, b"false", HOST)),
    ((b"X", b"m1", P, b'{"topic":null}'), (COMMIT, HEADERS, K_NULL, b"null", HOST)),
    ((b"X", b"m1", P, b'{"topic":""}'), (COMMIT, HEADERS, K_STR, b"", 6)),
    ((b"X", b"m1", P, b'{"topic":"gamma"}'), (COMMIT, HEADERS, K_STR, b"gamma", UNKNOWN)),
    ((b"X", b"m1", P, b'{"topic":"alph"}'), (COMMIT, HEADERS, K_STR, b"alph", UNKNOWN)),
    ((b"X", b"m1", P, b'{"topic":"alphaa"}'), (COMMIT, HEADERS, K_STR, b"alphaa", UNKNOWN)),
]


def hand_records():
    return [T.tm_wire([b"orders", ty, mid, pl, hd], 1_000 + i) for i, ((ty, mid, pl, hd), _) in enumerate(HAND)]


def check_hand(out, data, rec_off, first=0):
    """out (any classifier's) against the hand table's expectations, records first .. first+len(HAND)."""
    for j, (fields, (cm, src, kind, tok, idx)) in enumerate(HAND):
        i = first + j
        got = (int(out["cm"][i]), int(out["topic_src"][i]), int(out["topic_kind"][i]), int(out["topic_idx"][i]))
        assert got == (cm, src, kind, idx), (j, fields, got)
        o, ln = int(out["topic_off"][i]), int(out["topic_len"][i])
        if tok is None:
            assert (o, ln) == (0, 0), (j, fields, o, ln)
        else:
            b = int(rec_off[i])
            assert bytes(data[b + o: b + o + ln]) == tok and ln == len(tok), (j, fields, o, ln)


# ------------------------------------------------------------------------------------------
# seeded random batch: short records of every category
# ------------------------------------------------------------------------------------------
_NAMES = [b"alpha", b"beta", b"gamma", b"orders", b"_ack", b"_subscriptions", b"_control", b"_control", b""]
_TYPES = [b"CREATE_ORDER", b"UPDATE_ORDER", b"REPLAY_COMPLETE", b"X", b"", b"SUBSCRIBE", b"COMMIT_RESPONSE",
          b"acknowledgment", b"Acknowledgment_legacy", b"Acknowledgment", b"acknowledgment_legacy", b"SUBSCRIBf"]


def _jstr(r, s: bytes) -> bytes:
    out = b""
    for ch in s:
        k = r.random()
        if k < 0.08:
            out += b"\\u%04x" % ch
        elif ch == ord('"'):
            out += b'\\"'
        else:
            out += bytes([ch])
    return b'"' + out + b'"'


def _topic_value(r) -> bytes:
    k = r.random()
    if k < 0.72:
        return _jstr(r, r.choice(_NAMES))
    if k < 0.80:
        return r.choice([b"12", b"-3.5", b"1e2", b"true", b"false", b"null"])
    if k < 0.90:
        return r.choice([b"[]", b'{"topic":"alpha"}', b'["beta"]', b"{}"])
    return r.choice([b'"alp', b"1e", b"tru", b'"a\\q"', b"-"])


def _filler(r) -> bytes:
    return r.choice([b'"qty":7', b'"side":"BUY"', b'"note":"a topic here"', b'"e":"x\\ny"', b'"arr":[1,{"topic":"no"}]',
                     b'"k":"REPLAY_COMPLETE"', b'"t":null'])


def _doc(r, where: int) -> bytes:
    """where: 0 no topic, 1 root topic, 2 message.topic, 3 both"""
    k = r.random()
    if k < 0.04:
        return r.choice([b"", b"null", b"[1]", b'"topic"', b"7", b"{", b'{"a":'])
    members = [_filler(r) for _ in range(r.randrange(0, 3))]
    key = b'"t\\u006fpic"' if r.random() < 0.1 else b'"topic"'
    if where & 1:
        members.insert(r.randrange(len(members) + 1), key + b":" + _topic_value(r))
        if r.random() < 0.08:
            members.append(key + b": " + _topic_value(r))
    if where & 2:
        inner = [_filler(r) for _ in range(r.randrange(0, 2))] + [key + b":" + _topic_value(r)]
        r.shuffle(inner)
        m = b'"message":{' + b",".join(inner) + b"}"
        members.insert(r.randrange(len(members) + 1), m)
        if r.random() < 0.06:
            members.append(r.choice([b'"message":1', b'"message":{"topic":"gamma"}']))
    elif r.random() < 0.1:
        members.append(r.choice([b'"message":"topic"', b'"message":null', b'"message":[{"topic":"x"}]']))
    d = b"{" + b",".join(members) + b"}"
    k = r.random()
    if k < 0.05:
        d = b"/* c */ " + d + b" // topic"
    elif k < 0.08:
        d = d[:-1] + b",}"
    elif k < 0.11:
        j = r.randrange(len(d) + 1)
        d = d[:j] + r.choice([b"\0", b",", b"\\", b'"']) + d[j:]
    return d


def random_records(n: int, seed: int):
    r = random.Random(seed)
    recs = []
    for i in range(n):
        c = r.random()
        if c < 0.04:
            recs.append(T.ack_wire(b"ack_%d" % i, b"orders", b"c", 5 + i))
            continue
        if c < 0.07:
            recs.append(T.session_event(i, 9, 7, 1, 0, b"detail"))
            continue
        if c < 0.10:
            recs.append(r.choice([b"", b"\x01\x02", T.hdr_bytes(16, 77, 1, 1) + b"\0" * 16, T.hdr_bytes(16, 1, 1, 1)]))
            continue
        ty = r.choice(_TYPES) if r.random() < 0.35 else b"CREATE_ORDER"
        mid = b"" if r.random() < 0.12 else (b"ack_%d" % i if r.random() < 0.08 else b"msg_%d" % i)
        hw = r.choice([0, 0, 0, 1, 1])
        pw = r.choice([0, 0, 1, 2, 2, 3])
        hd = r.choice([b"", b"{}"]) if r.random() < 0.15 else _doc(r, hw)
        pl = b"" if r.random() < 0.12 else _doc(r, pw)
        rec = T.tm_wire([r.choice([b"orders", b"t"]), ty, mid, pl, hd], 10_000 + i)
        if r.random() < 0.1:
            rec = T.session_wrap(rec)
        if r.random() < 0.02:  # headers cut short: SBE_FL_HEADERS_E100
            rec = rec[: len(rec) - len(hd) // 2 - 1] if hd else rec
        recs.append(rec)
    return recs
