"""Sequential model of sbe_order_select (include/sbecodec.h) and the edge batch its tests share.

The model restates ParseResult::is_session_event / is_topic_message / is_acknowledgment /
is_order_message (include/aeron_cluster/sbe_messages.hpp:332-406) and classify_topic
(include/aeron_cluster/topic_router.hpp) over Python bytes, with the `in` operator for every
substring test.  Which strings and header fields a record's ParseResult has follows the host
mirror's materialize_into; every view is first kept inside its record, as the kernels keep it."""
import ctypes
import os
import struct
import subprocess

import numpy as np

import sbe_testlib as T

ST_TM, ST_ACK, ST_SESSION_EVENT = 0, 1, 2
ST_ERR_FIRST, ST_ERR_UNKNOWN_TYPE, ST_ERR_LAST = 16, 18, 26
FL_PAYLOAD_DEFAULT = 0x2
PR_SESSION_EVENT, PR_TOPIC_MESSAGE, PR_ACKNOWLEDGMENT, PR_ORDER_MESSAGE = 1, 2, 4, 8
TC_UNKNOWN, TC_ORDERS, TC_CONTROL = 0, 1, 2

NEEDLES = (b"order_details", b"token_pair", b"quantity", b"side", b"client_order_id")
TOPICS_ORDERS = (b"orders", b"order_request_topic")
TOPICS_CONTROL = (b"_subscriptions", b"_ack", b"_control", b"_internal")


def clamped(L, off, ln):
    """A view kept inside a record of L bytes (sbe_delivery_keys, sbe_commit_kernel)."""
    o = min(int(off), L)
    return o, min(int(ln), L - o)


def parse_result(rec: bytes, st, fl, hdr, vo, vl):
    """(template_id, schema_id, message_type, payload) of the record's ParseResult, or None when the
    parse mode produces no such status."""
    def view(k):
        o, l = clamped(len(rec), vo[k], vl[k])
        return rec[o:o + l]
    if st == ST_TM:
        return int(hdr[1]), int(hdr[2]), view(1), view(3)
    if st == ST_ACK:
        return int(hdr[1]), int(hdr[2]), b"Acknowledgment", b"SUCCESS" if fl & FL_PAYLOAD_DEFAULT else view(1)
    if st == ST_SESSION_EVENT:
        return int(hdr[1]), int(hdr[2]), b"SessionEvent", view(3)
    if st == ST_ERR_UNKNOWN_TYPE:
        return int(hdr[1]), int(hdr[2]), b"", b""
    if ST_ERR_FIRST <= st <= ST_ERR_LAST:
        return 0, 0, b"", b""
    return None


def is_session_event(t, s, mtype, payload):  # sbe_messages.hpp:332-335
    return t == 2 and s == 111


def is_topic_message(t, s, mtype, payload):  # :340-369
    if t == 1 and (s == 1 or s == 1):
        return True
    if s == 111 and t == 1:
        return True
    if s == 1 and t == 2:
        return True
    if mtype and (b"ORDER" in mtype or b"TopicMessage" in mtype or b"CREATE_ORDER" in mtype or b"UPDATE_ORDER" in mtype):
        return True
    return False


def is_acknowledgment(t, s, mtype, payload):  # :374-377
    return t == 2 and s == 1


def is_order_message(t, s, mtype, payload):  # :382-406
    if is_topic_message(t, s, mtype, payload):
        if mtype and (mtype == b"CREATE_ORDER" or b"ORDER" in mtype or b"CREATE_ORDER" in mtype or
                      b"UPDATE_ORDER" in mtype or b"CANCEL_ORDER" in mtype):
            return True
        if payload and (b"order_details" in payload or b"token_pair" in payload or b"quantity" in payload or
                        b"side" in payload or b"client_order_id" in payload):
            return True
    return False


def classify_topic(topic: bytes):  # topic_router.hpp
    if topic in TOPICS_ORDERS:
        return TC_ORDERS
    if topic in TOPICS_CONTROL:
        return TC_CONTROL
    return TC_UNKNOWN


def model(data, rec_off, dec):
    """Every output of sbe_order_select: dict(pred, select, topic_class, totals)."""
    buf = bytes(np.asarray(data, np.uint8))
    rec_off = np.asarray(rec_off, np.uint64)
    n = rec_off.size - 1
    pred, sel, tc = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        b, e = int(rec_off[i]), int(rec_off[i + 1])
        rec = buf[b:e] if e > b else b""
        st = int(dec["status"][i])
        pr = parse_result(rec, st, int(dec["flags"][i]), dec["hdr"][i], dec["view_off"][i], dec["view_len"][i])
        if pr is not None:
            pred[i] = (PR_SESSION_EVENT * is_session_event(*pr) | PR_TOPIC_MESSAGE * is_topic_message(*pr) |
                       PR_ACKNOWLEDGMENT * is_acknowledgment(*pr) | PR_ORDER_MESSAGE * is_order_message(*pr))
        if st == ST_TM:
            sel[i] = 1 if pred[i] & PR_ORDER_MESSAGE else 0
            o, l = clamped(len(rec), dec["view_off"][i][0], dec["view_len"][i][0])
            tc[i] = classify_topic(rec[o:o + l])
    totals = np.array([int(sel.sum()), int(((pred & PR_ORDER_MESSAGE) != 0).sum())], np.uint64)
    return {"pred": pred, "select": sel, "topic_class": tc, "totals": totals}


# ------------------------------------------------------------------------------------------
# the edge batch
# ------------------------------------------------------------------------------------------
def tm(topic=b"t", mtype=b"", uuid=b"u", payload=b"", headers=b"{}", ts=7):
    return T.tm_wire([topic, mtype, uuid, payload, headers], ts)


def payload_pos(topic=b"t", mtype=b"", uuid=b"u"):
    """Offset of the payload's first byte in a tm() record."""
    return 24 + 2 + len(topic) + 2 + len(mtype) + 2 + len(uuid) + 2


def type_pos(topic=b"t"):
    return 24 + 2 + len(topic) + 2


def filler():
    """A TopicMessage no clause selects and no search is run for (empty type, empty payload)."""
    return tm(headers=b'{"pad":1}')


def edge_batch(window: int):
    """[(name, record)] of the smallest shapes at which the kernel can go wrong; `window` is
    sbe_order_select_window().  The order matters: see the tile notes at the end."""
    W = window
    out = [("odd_start", tm(payload=b"xyz"))]  # 44 bytes: the records behind it start off 16

    # chunk splits: every needle, and ORDER in the type, at each of the 16 alignments of its first
    # byte relative to the record start; and a twin that misses by its last byte
    for nd in NEEDLES:
        for j in range(16):
            pad = (j - payload_pos()) % 16
            out.append((f"split_{nd.decode()}_{j}", tm(payload=b"x" * pad + nd + b"yy")))
            out.append((f"split_miss_{nd.decode()}_{j}", tm(payload=b"x" * pad + nd[:-1] + b"#yy")))
    for j in range(16):
        pad = (j - type_pos()) % 16
        out.append((f"split_ORDER_{j}", tm(mtype=b"x" * pad + b"ORDER")))
        out.append((f"split_miss_ORDER_{j}", tm(mtype=b"x" * pad + b"ORDEr", payload=b"{}")))

    # view edges: first bytes, last bytes, the whole payload
    for nd in NEEDLES:
        out.append((f"first_{nd.decode()}", tm(payload=nd + b"zzz")))
        out.append((f"last_{nd.decode()}", tm(payload=b"zzz" + nd)))
        out.append((f"whole_{nd.decode()}", tm(payload=nd)))

    # short by one byte; wrong case
    for s in (b"sid", b"ide", b"quantit", b"uantity", b"client_order_i", b"order_detail", b"token_pai"):
        out.append((f"short_{s.decode()}", tm(payload=s)))
        out.append((f"short_mid_{s.decode()}", tm(payload=b'{"' + s + b'":1}')))
    for s in (b"Side", b"SIDE", b"order"):
        out.append((f"case_payload_{s.decode()}", tm(payload=s)))
    for s in (b"order", b"Order", b"topicmessage"):
        out.append((f"case_type_{s.decode()}", tm(mtype=s, payload=b"{}")))

    # spliced by a length prefix: 121 is 'y', 26995 is 's' 'i', 82 is 'R'
    out.append(("splice_payload_end", tm(payload=b"{}quantit", headers=b"h" * 121)))
    out.append(("splice_payload_end_twin", tm(payload=b"{}quantity", headers=b"h" * 121)))
    out.append(("splice_payload_start", tm(payload=b"de" + b"x" * 26993)))
    out.append(("splice_type_end", tm(mtype=b"ORDE", uuid=b"u" * 82)))

    # window straddles.  A spacer (not searched: its bulk is in the headers) of more than a window
    # in front of each record makes it the first one its rounds look at, so the window edges fall
    # at payload offsets W - lead and 2 W - 16 - lead, lead = the payload's address mod 16.
    def straddle(name, at, nd, k):
        out.append((f"spacer_{name}", tm(headers=b"x" * (W + 64))))
        body = bytearray(b"x" * (2 * W + 64))
        if nd:
            body[at:at + len(nd)] = nd
        out.append((name, tm(uuid=b"u" * (k % 16), payload=bytes(body))))
    for j in range(16):
        straddle(f"straddle_w_{j}", W - j, NEEDLES[j % 5], j)
        straddle(f"straddle_2w_{j}", 2 * W - j, NEEDLES[(j + 2) % 5], 3 * j + 1)
        straddle(f"straddle_2w_edge_{j}", 2 * W - 32 - j, NEEDLES[4 * (j & 1)], 5 * j + 2)
    straddle("straddle_none", 0, b"", 9)

    # records that are not TopicMessages
    for k in range(12):
        out.append((f"ack_default_{k}", T.simple_ack(1_000_000_000_000 + k)))
        out.append((f"ack_needle_{k}", T.ack_wire(b"msg_%d" % k, b"xx" + NEEDLES[k % 5] + b"xx", b"corr-1", 77 + k) + b"\0" * 8))
    out.append(("ack_plain", T.ack_wire(b"msg_1", b"orders", b"corr-1", 77) + b"\0" * 8))
    for k in range(11):
        out.append((f"session_event_{k}", T.session_event(k, 2, 3, 4, k % 3, detail=NEEDLES[k % 5] if k % 2 else b"redirect")))
    for name, rec in T.edge_records():
        if not name.startswith(("tm_prefix", "wrapped_prefix", "ack_prefix", "random")):
            out.append(("edge_" + name, rec))
    out.append(("wrapped_needle", T.session_wrap(tm(payload=b'{"quantity":1}'))))
    out.append(("wrapped_type", T.session_wrap(tm(mtype=b"CANCEL_ORDER"))))
    out.append(("wrapped_none", T.session_wrap(tm(payload=b"{}"))))

    # empties
    out.append(("empty_type_empty_payload", tm()))
    out.append(("topicmessage_empty_payload", tm(mtype=b"TopicMessage")))
    out.append(("topicmessage_payload", tm(mtype=b"xTopicMessagex", payload=b'{"side":1}')))
    out.append(("order_type_empty_payload", tm(mtype=b"UPDATE_ORDER")))

    # topic classes
    for name in TOPICS_ORDERS + TOPICS_CONTROL:
        out.append((f"topic_{name.decode()}", tm(topic=name, payload=b"{}")))
        out.append((f"topic_plus_{name.decode()}", tm(topic=name + b"s", payload=b"{}")))
        out.append((f"topic_minus_{name.decode()}", tm(topic=name[:-1], payload=b"{}")))
    out.append(("topic_empty", tm(topic=b"", payload=b"{}")))

    # tile positions: fill up to a tile boundary; a tile of 64 CREATE_ORDER records (no search);
    # a tile whose lanes 0 and 63 alone need the search; a last, partial tile with the decisive
    # records first and last
    while len(out) % 64:
        out.append((f"pad_{len(out)}", filler()))
    for k in range(64):
        out.append((f"create_order_{k}", tm(topic=b"orders", mtype=b"CREATE_ORDER", uuid=b"id_%d" % k, payload=b'{"px":%d}' % k)))
    out.append(("lane0_needle", tm(payload=b'{"token_pair":"a"}')))
    for k in range(62):
        out.append((f"mid_{k}", tm(mtype=b"CREATE_ORDER", payload=b"{}") if k % 2 else filler()))
    out.append(("lane63_needle", tm(payload=b'{"client_order_id":"a"}')))
    out.append(("tail_first", tm(payload=b'{"side":"BUY"}')))
    for k in range(5):
        out.append((f"tail_mid_{k}", tm(payload=b'{"sid":"BUY"}')))
    out.append(("tail_last", tm(payload=b'{"order_details":{}}')))
    return out


def edge_case(window: int):
    """(names, data, rec_off, dec) of the edge batch, decoded by the oracle."""
    batch = edge_batch(window)
    data, rec_off = T.pack_records([r for _, r in batch])
    return [n for n, _ in batch], data, rec_off, T.oracle_decode(data, rec_off, T.DEC_PARSE)


def check_composition(names, data, rec_off, dec, exp, window):
    """The batch means something under the model alone."""
    n = len(names)
    pred, sel = exp["pred"], exp["select"]
    for bit in (PR_SESSION_EVENT, PR_TOPIC_MESSAGE, PR_ACKNOWLEDGMENT, PR_ORDER_MESSAGE):
        on = int(((pred & bit) != 0).sum())
        assert on >= 10 and n - on >= 10, (bit, on, n)
    is_tm = dec["status"] == ST_TM
    ntm = int(is_tm.sum())
    assert 3 * int(sel[is_tm].sum()) >= ntm and 3 * int((sel[is_tm] == 0).sum()) >= ntm, (int(sel.sum()), ntm)
    at = {nm: i for i, nm in enumerate(names)}
    assert len(at) == n
    # what each group is there to show
    for nm, i in at.items():
        if nm.startswith(("split_miss_", "short_", "case_", "spacer_")) or nm in ("splice_payload_end", "splice_payload_start",
                                                                               "splice_type_end", "straddle_none"):
            assert sel[i] == 0 and dec["status"][i] == ST_TM, nm
        elif nm.startswith(("split_", "first_", "last_", "whole_", "straddle_", "create_order_", "lane")) or \
                nm == "splice_payload_end_twin":
            assert sel[i] == 1, nm
        elif nm.startswith("ack_needle_"):
            assert dec["status"][i] == ST_ACK and pred[i] == PR_TOPIC_MESSAGE | PR_ACKNOWLEDGMENT | PR_ORDER_MESSAGE and not sel[i], nm
        elif nm.startswith("ack_default_"):
            assert dec["status"][i] == ST_ACK and dec["flags"][i] & FL_PAYLOAD_DEFAULT and pred[i] == 6, nm
        elif nm.startswith("session_event_"):
            assert dec["status"][i] == ST_SESSION_EVENT and pred[i] == PR_SESSION_EVENT, nm
    assert pred[at["topicmessage_empty_payload"]] == PR_TOPIC_MESSAGE and pred[at["empty_type_empty_payload"]] == PR_TOPIC_MESSAGE
    for nm in ("wrapped_needle", "wrapped_type"):  # a schema-111 frame; its ParseResult has the embedded header
        assert dec["flags"][at[nm]] & 0x10 and data[int(rec_off[at[nm]]) + 4] == 111 and sel[at[nm]], nm
    assert dec["flags"][at["wrapped_none"]] & 0x10 and pred[at["wrapped_none"]] == PR_TOPIC_MESSAGE
    st = set(int(s) for s in dec["status"])  # every error status the generators produce
    gd, go = T.pack_records([r for _, r in T.edge_records()])
    gen = set(int(s) for s in T.oracle_decode(gd, go, T.DEC_PARSE)["status"])
    assert gen <= st and len([s for s in st if s >= ST_ERR_FIRST]) >= 8, (sorted(gen), sorted(st))
    assert any(dec["status"][i] == ST_ERR_UNKNOWN_TYPE and dec["hdr"][i][1] for i in range(n))
    # the splices spell the rest of a needle with a length prefix
    i = at["splice_payload_end"]
    o, l = int(dec["view_off"][i][3]), int(dec["view_len"][i][3])
    assert bytes(data[int(rec_off[i]) + o:int(rec_off[i]) + o + l + 1]).endswith(b"quantity")
    i = at["splice_payload_start"]
    o = int(rec_off[i]) + int(dec["view_off"][i][3])
    assert bytes(data[o - 2:o + 2]) == b"side"
    i = at["splice_type_end"]
    o = int(rec_off[i]) + int(dec["view_off"][i][1])
    assert bytes(data[o:o + 5]) == b"ORDER" and dec["view_len"][i][1] == 4
    # window straddles: with the batch at a 16-byte boundary, needles lie across the first and
    # the second window edge of their record
    cross = [0, 0]
    for nm, i in at.items():
        if not nm.startswith("straddle_") or nm == "straddle_none":
            continue
        s = int(rec_off[i]) + int(dec["view_off"][i][3])
        body = bytes(data[s:s + int(dec["view_len"][i][3])])
        pos, ln = next((body.find(nd), len(nd)) for nd in NEEDLES if nd in body)
        for e, edge in enumerate((window - s % 16, 2 * window - 16 - s % 16)):
            cross[e] += pos < edge < pos + ln
    assert cross[0] >= 4 and cross[1] >= 4, cross
    # tile positions
    t = at["create_order_0"]
    assert t % 64 == 0 and at["lane0_needle"] == t + 64 and at["lane63_needle"] == t + 127 and at["tail_first"] == t + 128
    assert n % 64 and at["tail_last"] == n - 1 and sel[at["tail_first"]] and sel[n - 1]
    assert rec_off[1] % 16 and len(set(int(o) % 16 for o in rec_off[:-1])) == 16


DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "select")
_libs = {}


def make(target):
    subprocess.run(["make", "-s", "-C", DIR, target], check=True)
    return os.path.join(DIR, target)


def window():
    """sbe_order_select_window() of the built library (no device needed)."""
    if "codec" not in _libs:
        _libs["codec"] = ctypes.CDLL(os.path.join(T.PKG, "libsbecodec.so"))
        _libs["codec"].sbe_order_select_window.restype = ctypes.c_uint32
    return int(_libs["codec"].sbe_order_select_window())


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def chk_select(data, rec_off, dec, win, base_lead=0, want_select=True, want_class=True):
    """The device search compiled for the host (tests/select/select_host_check.cpp) over a window
    of `win` bytes, with in[0] at an address of base_lead mod 16."""
    if "chk" not in _libs:
        _libs["chk"] = ctypes.CDLL(make("select_host_check.so"))
        _libs["chk"].chk_select.restype = ctypes.c_int
        _libs["chk"].chk_select.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint64] + [ctypes.c_void_p] * 5 + \
            [ctypes.c_uint32] * 2 + [ctypes.c_void_p] * 4
    n = len(rec_off) - 1
    m = max(n, 1)
    buf = np.ascontiguousarray(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    ro = np.ascontiguousarray(rec_off, np.uint64)
    arr = {k: np.ascontiguousarray(dec[k], t) for k, t in (("status", np.uint8), ("flags", np.uint8), ("hdr", np.uint16),
                                                            ("view_off", np.uint32), ("view_len", np.uint32))}
    out = {"pred": np.full(m, 0xEE, np.uint8), "select": np.full(m, 0xEE, np.uint8),
           "topic_class": np.full(m, 0xEE, np.uint8), "totals": np.zeros(2, np.uint64)}
    rc = _libs["chk"].chk_select(_p(buf), _p(ro), n, _p(arr["status"]), _p(arr["flags"]), _p(arr["hdr"]),
                                 _p(arr["view_off"]), _p(arr["view_len"]), win, base_lead, _p(out["pred"]),
                                 _p(out["select"]) if want_select else None,
                                 _p(out["topic_class"]) if want_class else None, _p(out["totals"]))
    assert rc == 0, rc
    return {k: (v if k == "totals" else v[:n]) for k, v in out.items()}


def same(got, exp, what, names=None, keys=("pred", "select", "topic_class", "totals")):
    for k in keys:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        bad = np.nonzero(g != e)[0]
        assert bad.size == 0, (what, k, [(int(i), names[i] if names and k != "totals" else "", int(g[i]), int(e[i])) for i in bad[:8]])


def write_case(path, data, rec_off, dec, exp, win, base_lead):
    """A case file of tests/select/select_sanitize_main.cpp."""
    n = len(rec_off) - 1
    with open(path, "wb") as f:
        f.write(struct.pack("<5Q", 0x31304C45534F4253, n, len(data), win, base_lead))
        for a, t in ((data, np.uint8), (rec_off, np.uint64), (dec["status"], np.uint8), (dec["flags"], np.uint8),
                     (dec["hdr"], np.uint16), (dec["view_off"], np.uint32), (dec["view_len"], np.uint32),
                     (exp["pred"], np.uint8), (exp["select"], np.uint8), (exp["topic_class"], np.uint8)):
            f.write(np.ascontiguousarray(a, t).tobytes())


def mutated_case(n, seed):
    """n records of the existing generators with keywords spliced into types and payloads."""
    rng = np.random.default_rng(seed)
    data, off = T.mixed_records(n, seed)
    data = data.copy()
    words = NEEDLES + (b"ORDER", b"TopicMessage", b"sid", b"Side", b"quantit", b"ORDE")
    types = (b"create_order", b"TopicMessage", b"xxxxORDERxxx", b"xxxxxxxxxxxx", b"abcdefghijkl")
    for i in range(n):
        b, e = int(off[i]), int(off[i + 1])
        if e - b != 256 or rng.integers(0, 4) == 0:
            continue
        # a fixed-256 Order: 12 bytes of type at 34 (CREATE_ORDER), 143 bytes of payload at 79,
        # which begins {"side": the template's own needles go
        data[b + 34:b + 46] = np.frombuffer(types[int(rng.integers(0, len(types)))], np.uint8)
        data[b + 81:b + 85] = np.frombuffer(b"SIDE", np.uint8)
        c = b + 79 + T._PAYLOAD_T.index(b"client_order_id")
        data[c:c + 15] = np.frombuffer(b"CLIENT_ORDER_ID", np.uint8)
        if rng.integers(0, 3) == 0:
            continue
        w = words[int(rng.integers(0, len(words)))]
        if rng.integers(0, 4):
            p = b + 79 + int(rng.integers(0, 143 - len(w) + 1))
        else:  # at the payload's end, or up to two bytes across it
            p = b + 79 + 143 - len(w) + int(rng.integers(0, 3))
        data[p:p + len(w)] = np.frombuffer(w, np.uint8)
    return data, off, T.oracle_decode(data, off, T.DEC_PARSE)
