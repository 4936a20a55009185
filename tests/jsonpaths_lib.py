"""Shared by test_jsonpaths_ref.py (CPU) and test_gpu_jsonpaths.py: the hand table, the seeded
random documents and the ctypes front ends of tests/jsonpaths (the reference restatement
paths_ref.so, the older copy of its reader paths_pin.so and the host build of the device walk
paths_host_check.so)."""
import ctypes
import os
import random
import subprocess

import numpy as np

import sbe_testlib as T

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jsonpaths")

OK, NOT_SELECTED, EMPTY, FAILED, STACK = range(5)
MISSING, STR, ESC, NUM, TRUE, FALSE, NULL, OBJ, ARR = range(9)
KEYS = ("doc", "root_kind", "kind", "off", "len")
ORDER_ID_PATHS = ["message", "message.message", "message.message.client_order_id", "message.message.order_id",
                  "message.message.order_details", "message.message.order_details.client_order_id",
                  "message.order_details", "message.order_details.client_order_id", "uuid"]

_libs = {}


def make(target):
    subprocess.run(["make", "-s", "-C", DIR, target], check=True)
    return os.path.join(DIR, target)


def _lib(name):
    if name not in _libs:
        _libs[name] = ctypes.CDLL(make(name + ".so"))
    return _libs[name]


def _dump(lib, fn, doc: bytes):
    f = getattr(_lib(lib), fn)
    f.restype = ctypes.c_uint64
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_uint64]
    cap = 64 * len(doc) + 256
    buf = ctypes.create_string_buffer(cap)
    verdict = ctypes.c_uint32(9)
    src = np.frombuffer(doc, np.uint8) if doc else np.zeros(1, np.uint8)
    n = int(f(src.ctypes.data_as(ctypes.c_void_p), len(doc), ctypes.byref(verdict), buf, cap))
    assert n <= cap, (n, cap)
    return verdict.value, buf.raw[:n]


def ref_dump(doc):
    """(verdict, canonical dump of the tree) of the restatement's reader."""
    return _dump("paths_ref", "pref_dump", doc)


def pin_dump(doc):
    """The same of the older copy of the reader (tests/autocommit/commit_ref.cpp)."""
    return _dump("paths_pin", "cpin_dump", doc)


def path_table(paths):
    """(n_paths, depth u8, names u8, name_off u32): the host arrays of sbe_json_paths.  A path is a
    dotted str or a list of bytes names."""
    flat, depth = [], []
    for p in paths:
        parts = [q.encode() for q in p.split(".")] if isinstance(p, str) else [bytes(q) for q in p]
        depth.append(len(parts))
        flat += parts
    off = np.zeros(len(flat) + 1, np.uint32)
    off[1:] = np.cumsum([len(q) for q in flat])
    return len(depth), np.asarray(depth, np.uint8), np.frombuffer(b"".join(flat) + b"\0", np.uint8).copy(), off


def _extract(lib, fn, data, rec_off, dec, paths, view, select):
    P, depth, names, name_off = paths if isinstance(paths, tuple) else path_table(paths)
    data = np.ascontiguousarray(data, np.uint8)
    rec_off = np.ascontiguousarray(rec_off, np.uint64)
    n = rec_off.size - 1
    m, w = max(n, 1), max(P, 1)
    out = dict(doc=np.full(m, 0xEE, np.uint8), root_kind=np.full(m, 0xEE, np.uint8), kind=np.full((m, w), 0xEE, np.uint8),
               off=np.full((m, w), 0xEEEEEEEE, np.uint32), len=np.full((m, w), 0xEEEEEEEE, np.uint32))
    p = ctypes.c_void_p
    ptr = lambda a: None if a is None else a.ctypes.data_as(p)  # noqa: E731
    d = [None] * 4 if dec is None else [np.ascontiguousarray(dec[k]) for k in ("status", "flags", "view_off", "view_len")]
    sel = None if select is None else np.ascontiguousarray(select, np.uint8)
    f = getattr(_lib(lib), fn)
    f.restype = ctypes.c_int
    f.argtypes = [p, p, ctypes.c_uint64, p, p, p, p, ctypes.c_uint32, p, ctypes.c_uint32] + [p] * 8
    src = data if data.size else np.zeros(1, np.uint8)
    rc = f(ptr(src), ptr(rec_off), n, *(ptr(a) for a in d), view, ptr(sel), P, ptr(depth), ptr(names), ptr(name_off),
           *(ptr(out[k]) for k in KEYS))
    out = {k: v[:n] for k, v in out.items()}
    return rc, out


def ref_extract(data, rec_off, dec, paths, view=None, select=None):
    """The restatement (paths_ref.cpp) on host arrays: the expected outputs of sbe_json_extract_batch."""
    view = (0 if dec is None else 3) if view is None else view
    return _extract("paths_ref", "pref_extract", data, rec_off, dec, paths, view, select)[1]


def chk_extract(data, rec_off, dec, paths, view=None, select=None, rc=False):
    """The device walk compiled for the host (paths_host_check.cpp); rc=True: (its verdict, outputs)."""
    view = (0 if dec is None else 3) if view is None else view
    r, out = _extract("paths_host_check", "chk_extract", data, rec_off, dec, paths, view, select)
    if rc:
        return r, out
    assert r == 0, r
    return out


def _src(doc: bytes):
    return np.frombuffer(doc, np.uint8) if doc else np.zeros(1, np.uint8)


def ref_order_ids(payload: bytes):
    """(client_order_id, order_id) of the example's callback body on one payload (paths_ref.cpp)."""
    f = _lib("paths_ref").pref_order_ids
    f.restype = None
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    cap = 2 * len(payload) + 16
    buf, lens = ctypes.create_string_buffer(cap), (ctypes.c_uint64 * 2)()
    f(_src(payload).ctypes.data_as(ctypes.c_void_p), len(payload), buf, cap, lens)
    return buf.raw[: lens[0]], buf.raw[lens[0]: lens[0] + lens[1]]


def ref_parse_commit_offset(doc: bytes):
    """(code, topic, message_identifier, message_id, timestamp_nanos, sequence_number); code 0
    parsed, 1 the parse failure's exception, 2 another exception (the members are then None)."""
    f = _lib("paths_ref").pref_parse_commit_offset
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                  ctypes.POINTER(ctypes.c_uint64)]
    cap = 3 * len(doc) + 64
    buf, lens, nums = ctypes.create_string_buffer(cap), (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 2)()
    rc = f(_src(doc).ctypes.data_as(ctypes.c_void_p), len(doc), buf, cap, lens, nums)
    if rc:
        return (rc,) + (None,) * 5
    a, b = lens[0], lens[0] + lens[1]
    return 0, buf.raw[:a], buf.raw[a:b], buf.raw[b:b + lens[2]], int(nums[0]), int(nums[1])


def ref_convert(doc: bytes, key: bytes):
    """asString and asUInt64 of root.get(key, null) of an object document: (string or None when it
    throws, integer or None when it throws)."""
    f = _lib("paths_ref").pref_convert
    f.restype = ctypes.c_int
    ip, up = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ip, ctypes.c_char_p, ctypes.c_uint64, up, ip, up]
    cap = len(doc) + 64
    buf, sc, uc, sl, uv = ctypes.create_string_buffer(cap), ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = f(_src(doc).ctypes.data_as(ctypes.c_void_p), len(doc), key, ctypes.byref(sc), buf, cap, ctypes.byref(sl),
           ctypes.byref(uc), ctypes.byref(uv))
    assert rc == 0, (doc, rc)
    return (None if sc.value else buf.raw[: sl.value]), (None if uc.value else int(uv.value))


def unescape(tok: bytes) -> bytes:
    """decodeString of the bytes between the quotes of a string token that parsed."""
    out, i = bytearray(), 0
    simple = {ord('"'): 34, ord("\\"): 92, ord("/"): 47, ord("b"): 8, ord("f"): 12, ord("n"): 10, ord("r"): 13, ord("t"): 9}
    while i < len(tok):
        c = tok[i]
        i += 1
        if c != 92:
            out.append(c)
            continue
        x = tok[i]
        i += 1
        if x in simple:
            out.append(simple[x])
            continue
        cp = int(tok[i:i + 4], 16)
        i += 4
        if 0xD800 <= cp <= 0xDBFF:
            cp = 0x10000 + ((cp & 0x3FF) << 10) + (int(tok[i + 2:i + 6], 16) & 0x3FF)
            i += 6
        out += chr(cp).encode("utf-8", "surrogatepass")
    return bytes(out)


def order_ids_from_fields(out, data, rec_off, i):
    """The order-id rule from the nine ORDER_ID_PATHS outputs of record i alone."""
    if out["doc"][i] != OK or out["root_kind"][i] != OBJ:
        return b"", b""
    kind = out["kind"][i]

    def find_str(p):
        if kind[p] not in (STR, ESC):
            return b""
        b = int(rec_off[i]) + int(out["off"][i][p])
        tok = bytes(data[b: b + int(out["len"][i][p])])
        return tok if kind[p] == STR else unescape(tok)

    coid = oid = b""
    if kind[0] == OBJ and kind[1] == OBJ:
        coid, oid = find_str(2), find_str(3)
        if not coid and kind[4] == OBJ:
            coid = find_str(5)
    elif kind[0] == OBJ and kind[6] == OBJ:
        coid = find_str(7)
    return coid, oid or find_str(8)


def same(got, exp, what="", data=None, off=None):
    for k in KEYS:
        assert got[k].shape == exp[k].shape, (what, k, got[k].shape, exp[k].shape)
        bad = np.nonzero((got[k] != exp[k]).reshape(got[k].shape[0], -1).any(axis=1))[0]
        ctx = [] if data is None else [bytes(data[int(off[i]):int(off[i + 1])])[:200] for i in bad[:3]]
        assert bad.size == 0, (what, k, bad[:5], got[k][bad[:3]], exp[k][bad[:3]], ctx)


# ------------------------------------------------------------------------------------------
# the hand table: document -> (doc code, root kind, {path: (kind, token bytes)}); a path that is
# not named is MISSING.  token: the bytes off / len must select in the document.
# ------------------------------------------------------------------------------------------
HAND_PATHS = ["a", "a.b", "a.b.c", "a.b.c.d", "s", "n", "t", "f", "z", "o", "r", "m.x", "m.y.z", "u", "a.e", "k.k.k.k"]
_VALUES = [(b'"v"', STR, b"v"), (b'"x\\ty"', ESC, b"x\\ty"), (b"-12.5e3", NUM, b"-12.5e3"), (b"true", TRUE, b"true"),
           (b"false", FALSE, b"false"), (b"null", NULL, b"null"), (b'{"q":[1]}', OBJ, b'{"q":[1]}'),
           (b'[{"b":1},2]', ARR, b'[{"b":1},2]')]
_DEEP_D = b"[" * 996 + b"]" * 996


def _spine(depth, text):
    """text as the value of a / a.b / a.b.c / a.b.c.d, and the expected OBJECT prefixes."""
    doc, exp = text, {}
    for d in range(depth, 0, -1):
        doc = b'{"%s":%s}' % (b"abcd"[d - 1:d], doc)
        if d > 1:
            exp[HAND_PATHS[d - 2]] = (OBJ, doc)
    return doc, exp


def _hand():
    h = []
    for d in range(1, 5):  # every kind at depths 1 to 4
        for text, kind, tok in _VALUES:
            doc, exp = _spine(d, text)
            exp[HAND_PATHS[d - 1]] = (kind, tok)
            h.append((doc, OK, OBJ, exp))
    A = lambda doc, exp=None, code=OK, root=OBJ: h.append((doc, code, root if code == OK else MISSING, exp or {}))  # noqa: E731
    # roots
    A(b"{}")
    A(b" { } ")
    A(b"null", root=NULL)
    A(b"7", root=NUM)
    A(b"-", root=NUM)
    A(b'"x"', root=STR)
    A(b'"x\\n"', root=ESC)
    A(b"[1,2]", root=ARR)
    A(b'[{"s":"v"}]', root=ARR)
    A(b"true", root=TRUE)
    A(b"false", root=FALSE)
    A(b"   ", code=FAILED)
    A(b"\0", code=FAILED)
    A(b"\xef\xbb\xbf", code=FAILED)
    # missing members, non-objects in the middle of a path
    A(b'{"q":1}')
    A(b'{"ab":1,"":2,"A":3}')
    A(b'{"a":[{"b":1}]}', {"a": (ARR, b'[{"b":1}]')})
    A(b'{"a":"str","s":"v"}', {"a": (STR, b"str"), "s": (STR, b"v")})
    A(b'{"a":{"b":5}}', {"a": (OBJ, b'{"b":5}'), "a.b": (NUM, b"5")})
    A(b'{"a":null,"n":0}', {"a": (NULL, b"null"), "n": (NUM, b"0")})
    A(b'{"a":{"b":[{"c":{"d":1}}]}}', {"a": (OBJ, b'{"b":[{"c":{"d":1}}]}'), "a.b": (ARR, b'[{"c":{"d":1}}]')})
    A(b'{"q":{"s":"v"},"s":"w"}', {"s": (STR, b"w")})
    A(b'{"s":"w","q":{"s":"v","a":{"b":1}}}', {"s": (STR, b"w")})
    A(b'{"m":{"x":1,"y":{"z":[1,{"z":2}]}}}', {"m.x": (NUM, b"1"), "m.y.z": (ARR, b'[1,{"z":2}]')})
    A(b'{"m":{"y":7,"x":"p"}}', {"m.x": (STR, b"p")})
    A(b'{"k":{"k":{"k":{"k":"deep"}}}}', {"k.k.k.k": (STR, b"deep")})
    A(b'{"k":{"k":{"k":{"k":{"k":1}}}}}', {"k.k.k.k": (OBJ, b'{"k":1}')})
    A(b'{"k":{"k":{"k":1}}}')
    A(b'{"o":{},"r":[]}', {"o": (OBJ, b"{}"), "r": (ARR, b"[]")})
    A(b'{"o":{ },"r":[ ]}', {"o": (OBJ, b"{ }"), "r": (ARR, b"[ ]")})
    A(b'{ "s" : "v" , "n" : 12 }', {"s": (STR, b"v"), "n": (NUM, b"12")})
    A(b'{"u":"\xc3\xa9\xe2\x82\xac","s":""}', {"u": (STR, b"\xc3\xa9\xe2\x82\xac"), "s": (STR, b"")})
    # duplicate keys: the last one wins at every level
    A(b'{"s":"1","s":"2"}', {"s": (STR, b"2")})
    A(b'{"a":{"b":1},"a":2}', {"a": (NUM, b"2")})
    A(b'{"a":2,"a":{"b":1}}', {"a": (OBJ, b'{"b":1}'), "a.b": (NUM, b"1")})
    A(b'{"a":{"b":{"c":1}},"a":{"e":2}}', {"a": (OBJ, b'{"e":2}'), "a.e": (NUM, b"2")})
    A(b'{"a":{"b":1,"b":[3]}}', {"a": (OBJ, b'{"b":1,"b":[3]}'), "a.b": (ARR, b"[3]")})
    A(b'{"a":{"b":{"c":{"d":1},"c":7}}}', {"a": (OBJ, b'{"b":{"c":{"d":1},"c":7}}'), "a.b": (OBJ, b'{"c":{"d":1},"c":7}'),
                                           "a.b.c": (NUM, b"7")})
    A(b'{"a":{"b":{"c":{"d":1,"d":"x"}}}}', {"a": (OBJ, b'{"b":{"c":{"d":1,"d":"x"}}}'), "a.b": (OBJ, b'{"c":{"d":1,"d":"x"}}'),
                                             "a.b.c": (OBJ, b'{"d":1,"d":"x"}'), "a.b.c.d": (STR, b"x")})
    A(b'{"a":{"b":1},"a":[],"a":{"b":2}}', {"a": (OBJ, b'{"b":2}'), "a.b": (NUM, b"2")})
    A(b'{"a":{"b":1,"e":2},"a":{}}', {"a": (OBJ, b"{}")})
    A(b'{"m":{"x":1},"m":5}')
    # escaped member names and values
    A(b'{"\\u0061":1}', {"a": (NUM, b"1")})
    A(b'{"a":{"\\u0062":"v"}}', {"a": (OBJ, b'{"\\u0062":"v"}'), "a.b": (STR, b"v")})
    A(b'{"s":"x\\"y"}', {"s": (ESC, b'x\\"y')})
    A(b'{"s":"\\ud83d\\ude00"}', {"s": (ESC, b"\\ud83d\\ude00")})
    A(b'{"a\\u0000":1,"\\u0061\\u0000":2}')
    A(b'{"\\/":1,"s\\n":2}')
    A(b'{"q\\q":1}', code=FAILED)
    A(b'{"s":"v","q":"\\x"}', code=FAILED)
    A(b'{"s":"\\ud800"}', code=FAILED)
    A(b'{"s":"\\u12"}', code=FAILED)
    # comments, trailing commas, BOM, content after the root, NUL
    A(b'/*c*/{"s":/*c*/"v"//y\n}', {"s": (STR, b"v")})
    A(b'{"s":"v"/*c*/,"n":1}', {"s": (STR, b"v"), "n": (NUM, b"1")})
    A(b'{"s"/*x*/:"v"}', code=FAILED)
    A(b'{"s":"v"}//', {"s": (STR, b"v")})
    A(b'{"s":"v" /* open', code=FAILED)
    A(b'{"s":"v",}', {"s": (STR, b"v")})
    A(b'{"r":[1,],}', {"r": (ARR, b"[1,]")})
    A(b"[1,]", root=ARR)
    A(b'{"s":"v",,}', code=FAILED)
    A(b"[,]", code=FAILED)
    A(b'\xef\xbb\xbf{"s":"v"}', {"s": (STR, b"v")})
    A(b'{"s":"v"} trailing {', {"s": (STR, b"v")})
    A(b'{"s":"v"}\0{', {"s": (STR, b"v")})
    A(b'{"s":\0"v"}', code=FAILED)
    A(b'{"s":"a\0b"}', {"s": (STR, b"a\0b")})
    # unterminated
    A(b'{"s":"v', code=FAILED)
    A(b'{"s":"v"', code=FAILED)
    A(b'{"a":{"b":1}', code=FAILED)
    A(b'"abc', code=FAILED)
    A(b"[1,2", code=FAILED)
    A(b'{"s":"v\\', code=FAILED)
    # numbers and literals
    A(b'{"n":-}', {"n": (NUM, b"-")})
    A(b'{"n":-x}', code=FAILED)
    A(b'{"n":1e}', code=FAILED)
    A(b'{"n":1.}', {"n": (NUM, b"1.")})
    A(b'{"n":-.5}', {"n": (NUM, b"-.5")})
    A(b'{"n":.5}', code=FAILED)
    A(b'{"n":01}', {"n": (NUM, b"01")})
    A(b'{"n":1E+5}', {"n": (NUM, b"1E+5")})
    A(b'{"n":12345678901234567890123}', {"n": (NUM, b"12345678901234567890123")})
    A(b'{"n":18446744073709551615,"z":-9223372036854775808}', {"n": (NUM, b"18446744073709551615"),
                                                                "z": (NUM, b"-9223372036854775808")})
    A(b'{"n":-Infinity}', code=FAILED)
    A(b'{"n":NaN}', code=FAILED)
    A(b'{"t":tru}', code=FAILED)
    A(b'{"t":truex}', code=FAILED)
    A(b'{"t":true,"f":false,"z":null}', {"t": (TRUE, b"true"), "f": (FALSE, b"false"), "z": (NULL, b"null")})
    # grammar
    A(b"{'s':'v'}", code=FAILED)
    A(b'{"s" "v"}', code=FAILED)
    A(b'{"s":}', code=FAILED)
    A(b"{s:1}", code=FAILED)
    A(b'{"s":1 "n":2}', code=FAILED)
    A(b"{1:2}", code=FAILED)
    A(b'{"r":[1 2]}', code=FAILED)
    A(b'{"r":[1}', code=FAILED)
    # the stack limit: a value inside 999 open containers is read, one inside 1000 throws
    A(b'{"s":"v","r":' + b"[" * 999 + b"]" * 999 + b"}", {"s": (STR, b"v"), "r": (ARR, b"[" * 999 + b"]" * 999)})
    A(b'{"s":"v","r":' + b"[" * 1000 + b"]" * 1000 + b"}", code=STACK)
    A(b"[" * 1000 + b"]" * 1000, root=ARR)
    A(b"[" * 1000 + b"1" + b"]" * 1000, code=STACK)
    A(b'{"a":{"b":{"c":{"d":' + _DEEP_D + b'}}},"s":"v"}',
      {"a": (OBJ, b'{"b":{"c":{"d":' + _DEEP_D + b"}}}"), "a.b": (OBJ, b'{"c":{"d":' + _DEEP_D + b"}}"),
       "a.b.c": (OBJ, b'{"d":' + _DEEP_D + b"}"), "a.b.c.d": (ARR, _DEEP_D), "s": (STR, b"v")})
    A(b'{"a":{"b":{"c":{"d":[' + _DEEP_D + b']}}},"s":"v"}', code=STACK)
    return h


HAND = _hand()


def hand_docs():
    return [d for d, _, _, _ in HAND]


def check_hand(out, data, rec_off, first=0, base=None):
    """out (anyone's, over HAND_PATHS) against the hand table's expectations, records first ..
    first + len(HAND); base[i]: where the document starts inside its record (default 0)."""
    for j, (doc, code, root, exp) in enumerate(HAND):
        i = first + j
        assert (int(out["doc"][i]), int(out["root_kind"][i])) == (code, root), (j, doc[:80], out["doc"][i], out["root_kind"][i])
        for p, name in enumerate(HAND_PATHS):
            kind, tok = exp.get(name, (MISSING, None))
            o, ln = int(out["off"][i][p]), int(out["len"][i][p])
            assert int(out["kind"][i][p]) == kind, (j, doc[:80], name, out["kind"][i][p])
            if tok is None:
                assert (o, ln) == (0, 0), (j, doc[:80], name, o, ln)
            else:
                b = int(rec_off[i])
                assert ln == len(tok) and bytes(data[b + o: b + o + ln]) == tok, (j, doc[:80], name, o, ln)
                if base is not None:
                    assert o >= int(base[i]), (j, name)


# ------------------------------------------------------------------------------------------
# hand cases of the two reference-anchored uses
# ------------------------------------------------------------------------------------------
_DEEP_UUID = b'{"uuid":"u","a":' + b"[" * 1000 + b"]" * 1000 + b"}"
# payload -> (client_order_id, order_id) of examples/pubsub_reconnect_test.cpp:582-623
ORDER_ID_CASES = [
    (b'{"message":{"message":{"client_order_id":"c1","order_id":"o1"}}}', (b"c1", b"o1")),
    (b'{"message":{"message":{"order_details":{"client_order_id":"c2"}}},"uuid":"u2"}', (b"c2", b"u2")),
    (b'{"message":{"message":{"client_order_id":"","order_details":{"client_order_id":"c3"}}}}', (b"c3", b"")),
    (b'{"message":{"message":{"client_order_id":"c4","order_details":{"client_order_id":"no"}}}}', (b"c4", b"")),
    (b'{"message":{"message":{"order_details":"x"}}}', (b"", b"")),
    (b'{"message":{"message":{"order_details":{"client_order_id":5}}}}', (b"", b"")),
    (b'{"message":{"message":5,"order_details":{"client_order_id":"c5"}}}', (b"c5", b"")),
    (b'{"message":{"message":null,"order_details":{"client_order_id":"c5n"}}}', (b"c5n", b"")),
    (b'{"message":{"order_details":{"client_order_id":"c6"}},"uuid":"u6"}', (b"c6", b"u6")),
    (b'{"message":{"message":{},"order_details":{"client_order_id":"c7"}}}', (b"", b"")),
    (b'{"message":{"order_details":["c"]},"uuid":"u7"}', (b"", b"u7")),
    (b'{"message":"x","uuid":"u8"}', (b"", b"u8")),
    (b'{"message":null,"uuid":"u8n"}', (b"", b"u8n")),
    (b'{"message":{"message":{"client_order_id":7,"order_id":true}}}', (b"", b"")),
    (b'{"uuid":5}', (b"", b"")),
    (b'{"uuid":""}', (b"", b"")),
    (b'{"message":{"message":{"order_id":"o9"}},"uuid":"u9"}', (b"", b"o9")),
    (b'{"message":{"message":{"order_id":""}},"uuid":"u10"}', (b"", b"u10")),
    (b'{"uuid":"a\\u0041\\n","message":{"message":{"cl\\u0069ent_order_id":"x\\"y"}}}', (b'x"y', b"aA\n")),
    (b'{"message":{"message":{"client_order_id":"x"}},"message":{"message":{"client_order_id":"y"}}}', (b"y", b"")),
    (b'{"message":{"message":{"client_order_id":"x"}},"message":1,"uuid":"u"}', (b"", b"u")),
    (b'{"message":{"message":{"client_order_id":"x"},"message":[]},"uuid":"u"}', (b"", b"u")),
    (b'{"uuid":"u","uuid":"v"}', (b"", b"v")),
    (b"{}", (b"", b"")),
    (b"null", (b"", b"")),
    (b'[{"uuid":"u"}]', (b"", b"")),       # isMember on an array throws
    (b'"uuid"', (b"", b"")),
    (b"7", (b"", b"")),
    (b'{"uuid":"u"', (b"", b"")),          # does not parse
    (b'{"uuid":"u"} trailing', (b"", b"u")),
    (_DEEP_UUID, (b"", b"")),              # the stack limit's exception
    (b"", (b"", b"")),
]
# value text X of {"v":X} -> (asString, asUInt64), None where the conversion throws
CONVERT_CASES = [
    (b"18446744073709551615", (b"18446744073709551615", 2 ** 64 - 1)),
    (b"18446744073709551616", (b"1.8446744073709552e+19", None)),
    (b"-1", (b"-1", None)),
    (b"1e19", (b"1e+19", 10 ** 19)),
    (b"1.5", (b"1.5", 1)),
    (b'"7"', (b"7", None)),
    (b"[]", (None, None)),
    (b"{}", (None, None)),
    (b"null", (b"", 0)),
    (b"true", (b"true", 1)),
    (b"false", (b"false", 0)),
    (b"0", (b"0", 0)),
    (b"-0", (b"0", 0)),
    (b"123", (b"123", 123)),
    (b"1.0", (b"1.0", 1)),
    (b"-0.0", (b"-0.0", 0)),
    (b"-0.5", (b"-0.5", None)),
    (b"1e20", (b"1e+20", None)),
    (b"9223372036854775808", (b"9223372036854775808", 2 ** 63)),
    (b"-9223372036854775808", (b"-9223372036854775808", None)),
    (b"18446744073709551615.0", (b"1.8446744073709552e+19", None)),
    (b"1e-3", (b"0.001", 0)),
    (b"0.1", (b"0.10000000000000001", 0)),
    (b'"a\\u00e9\\n"', (b"a\xc3\xa9\n", None)),
]
# document -> parse_commit_offset's code and members (src/commit_manager.cpp:177-195)
OFFSET_CASES = [
    (b'{"topic":"orders","message_identifier":"id1","message_id":"m1","timestamp_nanos":123,'
     b'"sequence_number":18446744073709551615}', (0, b"orders", b"id1", b"m1", 123, 2 ** 64 - 1)),
    (b'{"action":"COMMIT_OFFSET","messageIdentifier":"id","message_id":"m","sequence_number":7,"timestamp_nanos":9,'
     b'"topic":"t"}', (0, b"t", b"", b"m", 9, 7)),
    (b"{}", (0, b"", b"", b"", 0, 0)),
    (b"null", (0, b"", b"", b"", 0, 0)),
    (b'{"topic":5,"message_id":true,"message_identifier":null,"timestamp_nanos":1.5,"sequence_number":true}',
     (0, b"5", b"", b"true", 1, 1)),
    (b'{"topic":"a\\u0042","topic":"b\\n"}', (0, b"b\n", b"", b"", 0, 0)),
    (b'{"sequence_number":1e19}', (0, b"", b"", b"", 0, 10 ** 19)),
    (b'{"topic":"t"} and more', (0, b"t", b"", b"", 0, 0)),
    (b"[]", (2,)), (b"5", (2,)), (b'"topic"', (2,)),
    (b'{"topic":[]}', (2,)), (b'{"message_id":{}}', (2,)),
    (b'{"timestamp_nanos":-1}', (2,)), (b'{"sequence_number":"7"}', (2,)),
    (b'{"sequence_number":18446744073709551616}', (2,)), (b'{"timestamp_nanos":[]}', (2,)),
    (_DEEP_UUID, (2,)),
    (b'{"topic":', (1,)), (b"", (1,)), (b"{'topic':1}", (1,)), (b'{"timestamp_nanos":1e}', (1,)),
]


# ------------------------------------------------------------------------------------------
# seeded random documents over the names of HAND_PATHS
# ------------------------------------------------------------------------------------------
_NAMES = [b"a", b"b", b"c", b"d", b"s", b"n", b"m", b"x", b"y", b"z", b"k", b"o", b"r", b"u", b"e", b"t", b"f", b"q"]
PATHS_1 = ["a.b"]


def _key(r, name):
    if r.random() < 0.06:
        j = r.randrange(len(name))
        name = name[:j] + b"\\u%04x" % name[j] + name[j + 1:]
    return b'"' + name + b'"'


def _scalar(r):
    k = r.randrange(6)
    if k == 0:
        return b'"' + r.choice([b"", b"v", b"hello world", b"\xc3\xa9", b"{not json}"]) + b'"'
    if k == 1:
        return b'"' + r.choice([b"x\\ny", b'q\\"q', b"\\u0041", b"\\\\"]) + b'"'
    if k == 2:
        return r.choice([b"0", b"-1", b"12.5", b"1e9", b"-", b"18446744073709551615", b"-.5", b"3.25E-2"])
    return (b"true", b"false", b"null")[k - 3]


def _value(r, depth):
    k = r.random()
    if depth >= 5 or k < 0.55:
        return _scalar(r)
    if k < 0.85:
        return _object(r, depth + 1)
    return b"[" + b",".join(_value(r, depth + 1) for _ in range(r.randrange(0, 3))) + b"]"


def _object(r, depth):
    members = [_key(r, r.choice(_NAMES)) + b":" + _value(r, depth) for _ in range(r.randrange(0, 4))]
    return b"{" + b",".join(members) + b"}"


def _spine_doc(r):
    """One of the 16 paths spelled out, a random value at its end, random members around every level."""
    depth = r.randrange(1, 5)  # the depths equally often, whatever the table holds of each
    names = [q.encode() for q in r.choice([p for p in HAND_PATHS if p.count(".") == depth - 1]).split(".")]
    text = _value(r, len(names)) if r.random() < 0.8 else r.choice([b"{}", b"[]", b'{"b":1}', b"[[]]"])
    for d in range(len(names), 0, -1):
        members = [_key(r, r.choice(_NAMES)) + b":" + _value(r, d + 2) for _ in range(r.randrange(0, 3))]
        members.insert(r.randrange(len(members) + 1), _key(r, names[d - 1]) + b":" + text)
        text = b"{" + b",".join(members) + b"}"
    return text


def random_doc(r):
    k = r.random()
    if k < 0.025:
        return b""
    if k < 0.05:
        return r.choice([b"null", b"7", b'"s"', b"[1]", b"true", b"-", b"[]", b'"a\\tb"', b"false"])
    if k < 0.065:  # the stack limit, from both sides
        m = r.choice([990, 998, 999, 1000, 1003])
        return b'{"s":1,"a":{"b":' + b"[" * m + b"]" * m + b"}}"
    if k < 0.09:  # byte soup
        return bytes(r.choice(b'{}[]",:\\ \0abs10tfn/*-.e') for _ in range(r.randrange(1, 40)))
    d = _spine_doc(r) if k < 0.7 else _object(r, 1)
    k = r.random()
    if k < 0.04:
        d = b"/* c */ " + d + b" // s"
    elif k < 0.07:
        d = d[:-1] + b",}"
    elif k < 0.09:
        d = b"\xef\xbb\xbf" + d
    elif k < 0.11:
        d = d + r.choice([b" x", b"\0{", b"}"])
    elif k < 0.19:  # mangled
        j = r.randrange(len(d) + 1)
        if r.random() < 0.5:
            d = d[:j] + r.choice([b"\0", b",", b"\\", b'"', b"}", b"{", b":", b"/"]) + d[j:]
        else:
            d = d[:j] + d[j + 1:]
    return d


def random_docs(n, seed):
    r = random.Random(seed)
    return [random_doc(r) for _ in range(n)]


def random_select(n, seed, p=0.03):
    r = random.Random(seed)
    return np.array([0 if r.random() < p else r.choice([1, 1, 1, 2, 255]) for _ in range(n)], np.uint8)


def random_records(n, seed):
    """Mixed record kinds: TopicMessages with a random payload and random headers (some wrapped in
    a session frame, some cut short inside the headers), Acks, session events, error records."""
    r = random.Random(seed)
    recs = []
    for i in range(n):
        c = r.random()
        if c < 0.04:
            recs.append(T.ack_wire(b"ack_%d" % i, b"orders", b"c", 5 + i))
        elif c < 0.07:
            recs.append(T.session_event(i, 9, 7, 1, 0, b'{"s":"v"}'))
        elif c < 0.10:
            recs.append(r.choice([b"", b"\x01\x02", T.hdr_bytes(16, 77, 1, 1) + b"\0" * 16, T.hdr_bytes(16, 1, 1, 1)]))
        else:
            pl, hd = random_doc(r), random_doc(r)
            if len(pl) > 1500:
                pl = pl if r.random() < 0.5 else b'{"s":"v"}'
            rec = T.tm_wire([r.choice([b"orders", b"t"]), b"CREATE_ORDER", b"msg_%d" % i, pl, hd], 10_000 + i)
            if r.random() < 0.1:
                rec = T.session_wrap(rec)
            if r.random() < 0.03 and hd:  # headers cut short: SBE_FL_HEADERS_E100
                rec = rec[: len(rec) - len(hd) // 2 - 1]
            recs.append(rec)
    return recs
