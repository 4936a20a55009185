"""GPU: the host mirror on top of sbe_json_extract_batch (ParsedBatch::extract, JsonFields,
extract_json_documents, extract_order_ids, CommitManager::parse_commit_offset[s_batch]) through the
program tests/jsonpaths/test_jsonpaths_host.cpp, against the restatement tests/jsonpaths/paths_ref.cpp
and the hand cases of jsonpaths_lib."""
import struct
import subprocess

import numpy as np
import pytest

import jsonpaths_lib as J
import publish_lib as P
import sbe_testlib as T

pytestmark = pytest.mark.gpu


def _strs(items):
    return struct.pack("<I", len(items)) + b"".join(struct.pack("<I", len(s)) + bytes(s) for s in items)


class Reader:
    def __init__(self, raw):
        self.raw, self.at = raw, 0

    def u8(self):
        self.at += 1
        return self.raw[self.at - 1]

    def u64(self):
        self.at += 8
        return struct.unpack_from("<Q", self.raw, self.at - 8)[0]

    def s(self):
        n = struct.unpack_from("<I", self.raw, self.at)[0]
        self.at += 4 + n
        return self.raw[self.at - n: self.at]


def run(tmp_path, mode, blob):
    prog = J.make("test_jsonpaths_host")
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    r = subprocess.run([prog, mode, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "jsonpaths host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    return Reader(dst.read_bytes())


def _looked_at(msg_type: bytes, payload: bytes) -> bool:
    """is_order_message() || (is_topic_message() && message_type == "CREATE_ORDER") of a TopicMessage."""
    if b"ORDER" in msg_type:
        return True
    return bool(payload) and any(k in payload for k in (b"order_details", b"token_pair", b"quantity", b"side", b"client_order_id"))


def check_orders(tmp_path, recs, fields):
    """fields[i]: (message_type, payload, headers) of a TopicMessage record, or None."""
    out = run(tmp_path, "orders", _strs(recs))
    hits = 0
    for i, f in enumerate(fields):
        want = J.ref_order_ids(f[1]) if f and _looked_at(f[0], f[1]) else (b"", b"")
        got = (out.s(), out.s())
        assert got == want, (i, f and f[1][:120], got, want)
        hits += want != (b"", b"")
    data, off = T.pack_records(recs)
    dec = T.oracle_decode(data, off, T.DEC_PARSE)
    sel = np.array([i % 3 != 2 for i in range(len(recs))], np.uint8)
    exp = J.ref_extract(data, off, dec, ["messageType"], view=4, select=sel)
    for i in range(len(recs)):
        doc, kind, text = out.u8(), out.u8(), out.s()
        assert (doc, kind) == (exp["doc"][i], exp["kind"][i][0]), i
        if kind in (J.STR, J.ESC):
            b = int(off[i]) + int(exp["off"][i][0])
            tok = bytes(data[b: b + int(exp["len"][i][0])])
            assert text == (tok if kind == J.STR else J.unescape(tok)), i
    assert out.at == len(out.raw)
    return hits


def test_order_id_hand_cases(tmp_path):
    recs, fields = [], []
    for i, (payload, _) in enumerate(J.ORDER_ID_CASES):
        for ty in (b"CREATE_ORDER", b"UPDATE_ORDER", b"X", b"Acknowledgment"):
            hd = b'{"messageType":"%s"}' % ty if i % 2 else b'{"messageType":"\\u0041%d"}' % i
            recs.append(T.tm_wire([b"orders", ty, b"m%d" % i, payload, hd], i))
            fields.append((ty, payload, hd))
    recs += [T.ack_wire(b"ack_1", b"orders", b"c", 5), T.session_event(1, 9, 7, 1, 0, b'{"uuid":"u"}'), b"", b"\x01\x02"]
    fields += [None] * 4
    hits = check_orders(tmp_path, recs, fields)
    assert hits >= 2 * sum(1 for _, w in J.ORDER_ID_CASES if w != (b"", b""))  # the two ORDER types at least


def test_round_trip_edge_orders_through_the_mirror(codec, tmp_path):
    """2 000 edge Orders published on the device, then decode_batch + extract_order_ids in the host
    program: client_order_id and order_id (the uuid) are what the reference's callback extracts."""
    n = 2000
    fields, cid, ts, q = T.order_batch(n, 0xEDE, hard=True)
    for i in range(0, n, 37):
        fields[i][0] = b""
    z = np.zeros(n)
    b = P.Batch(fields, cid, ts, q, [b"LIMIT"] * n, [b"GTC"] * n, z, z, np.zeros(n, np.uint8))
    out, out_off, status, _ = P.run_device(codec, b, b"orders", None, 7, 1, True, 3, 4, validate=False)
    raw = out.tobytes()
    recs = [raw[int(out_off[i]):int(out_off[i + 1])] for i in range(n)]
    dec = T.oracle_decode(out[: int(out_off[-1])], out_off, T.DEC_PARSE)
    flds = []
    for i in range(n):
        if dec["status"][i] != T.ST_TM:
            flds.append(None)
            continue
        v = [recs[i][int(o):int(o) + int(ln)] for o, ln in zip(dec["view_off"][i], dec["view_len"][i])]
        flds.append((v[1], v[3], v[4]))
    hits = check_orders(tmp_path, recs, flds)
    # 55 Orders have an empty uuid (both ids empty by the rule) and a few dozen do not encode (E109)
    assert hits >= n - 55 - 100
    exact = 0
    for i in range(n):  # well-formed uuids come back as they went in
        try:
            fields[i][0].decode("utf-8")
        except UnicodeDecodeError:
            continue
        if flds[i] and fields[i][0]:
            assert J.ref_order_ids(flds[i][1]) == (fields[i][0], fields[i][0]), i
            exact += 1
    assert exact >= 1000


def test_fixed256_orders_through_the_mirror(tmp_path):
    n = 20000
    arena, L, ts = T.fixed256_orders(n)
    data, off, _ = T.oracle_encode(arena, L, ts)
    raw = data.tobytes()
    recs = [raw[int(off[i]):int(off[i + 1])] for i in range(n)]
    flds = [(r[34:46], r[79:222], r[224:256]) for r in recs]  # 24 B of header and fixed fields, then u16-prefixed strings
    assert flds[0][0] == b"CREATE_ORDER" and flds[0][1].startswith(b'{"side"') and flds[0][2].startswith(b'{"messageType"')
    assert check_orders(tmp_path, recs, flds) == 0  # flat payloads: no "message", no "uuid"


def test_fields_and_conversions(tmp_path):
    docs = [b'{"v":%s}' % t for t, _ in J.CONVERT_CASES] + [b'{"w":1}']
    out = run(tmp_path, "fields", struct.pack("<I", 1) + _strs([b"v"]) + _strs(docs))
    for doc, (_, (want_s, want_u)) in zip(docs, J.CONVERT_CASES + [(b"", (b"", 0))]):
        assert (out.u8(), out.u8()) == (J.OK, J.OBJ), doc
        out.u8(), out.u8(), out.s()
        s_code, s = out.u8(), out.s()
        u_code, u = out.u8(), out.u64()
        assert (None if s_code else s, None if u_code else u) == (want_s, want_u) == J.ref_convert(doc, b"v"), doc
    assert out.at == len(out.raw)
    # the hand table and random documents: every field of JsonFields against the restatement
    docs = J.hand_docs() + J.random_docs(600, 3)
    data, off = T.pack_records(docs)
    exp = J.ref_extract(data, off, None, J.HAND_PATHS)
    table = struct.pack("<I", 16) + b"".join(_strs([q.encode() for q in p.split(".")]) for p in J.HAND_PATHS)
    out = run(tmp_path, "fields", table + _strs(docs))
    for i, d in enumerate(docs):
        assert (out.u8(), out.u8()) == (exp["doc"][i], exp["root_kind"][i]), d[:80]
        for p in range(16):
            kind, is_str, tok = out.u8(), out.u8(), out.s()
            o, ln = int(exp["off"][i][p]), int(exp["len"][i][p])
            assert kind == exp["kind"][i][p] and tok == d[o:o + ln] and is_str == (kind in (J.STR, J.ESC)), (d[:80], p)
            s_code, s = out.u8(), out.s()
            out.u8(), out.u64()
            assert s_code == (kind in (J.OBJ, J.ARR)), (d[:80], p)
            if kind in (J.STR, J.ESC):
                assert s == (tok if kind == J.STR else J.unescape(tok)), (d[:80], p)
    assert out.at == len(out.raw)


def test_parse_commit_offsets(tmp_path):
    docs = [d for d, _ in J.OFFSET_CASES]
    out = run(tmp_path, "offsets", _strs(docs))
    for doc, want in J.OFFSET_CASES:
        got = (out.u8(), out.s(), out.s(), out.s(), out.u64(), out.u64())
        ref = J.ref_parse_commit_offset(doc)
        assert got[0] == want[0] == ref[0], (doc[:80], got)
        if got[0] == 0:
            assert got == want == ref, (doc[:80], got)
        else:
            assert got[1:] == (b"", b"", b"", 0, 0)
    assert out.at == len(out.raw)
