"""GPU: sbe_json_extract_batch, the JSON members a consumer's callback reads out of a decoded
payload (examples/pubsub_reconnect_test.cpp:576-620), by a caller-given table of paths.  Every
output array (doc, root_kind, kind, off, len) is compared bit-exactly with the restatement
tests/jsonpaths/paths_ref.cpp run over the oracle's decode of the same bytes (jsoncpp is absent:
parity with the library itself is unpinned, see test_jsonpaths_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

import contract_lib as C
import jsonpaths_lib as J
import publish_lib as P
import sbe_testlib as T
from test_gpu_contract import I32, U8, dec_inputs, dev, on_side_stream, _need
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu
WIN = 16384  # kJxWin of csrc/json_paths.hpp: the LDS window of a tile


def wrap(doc, i=0, headers=b"{}"):
    return T.tm_wire([b"t", b"X", b"m%d" % i, doc, headers], i)


def extract(codec, data, off, table, decoded=True, view=None, select=None):
    """GPU (decode +) extract of packed records; returns (got, expected, oracle decode)."""
    exp_dec = T.oracle_decode(data, off, T.DEC_PARSE) if decoded else None
    exp = J.ref_extract(data, off, exp_dec, table, view=view, select=select)
    d = to_dev(data if data.size else np.zeros(16, np.uint8), torch.uint8)
    ro = to_dev(np.asarray(off, np.uint64), torch.int64)
    dec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE) if decoded else None
    sel = None if select is None else to_dev(select, torch.uint8)
    got = codec.extract_json(d, ro, dec, table, view=view, select=sel)
    torch.cuda.synchronize()
    return got.numpy(), exp, exp_dec


def run(codec, recs, table=J.HAND_PATHS, lead=None, **kw):
    data, off = T.pack_records(([b"\0" * lead] if lead is not None else []) + recs)
    got, exp, dec = extract(codec, data, off, table, **kw)
    J.same(got, exp, "gpu", data, off)
    return got, data, off, dec


@pytest.mark.parametrize("lead", [0, 3, 9])
def test_hand_table(codec, lead):
    """The hand table as payloads, the batch shifted to three alignments."""
    got, data, off, dec = run(codec, [wrap(d, i) for i, d in enumerate(J.hand_docs())], lead=lead)
    assert got["doc"][0] == J.NOT_SELECTED  # the lead record
    J.check_hand(got, data, off, first=1, base=dec["view_off"][:, 3])


@pytest.mark.parametrize("lead", [0, 5])
def test_hand_table_bare_documents(codec, lead):
    """dec == NULL: every record is the document itself."""
    docs = J.hand_docs()
    got, data, off, _ = run(codec, docs, lead=lead, decoded=False)
    assert got["doc"][0] == (J.FAILED if lead else J.EMPTY)  # the lead record, NUL bytes
    J.check_hand(got, data, off, first=1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_tile_edges(codec, n):
    docs = J.random_docs(400, 17)
    recs = [wrap(d, i) for i, d in enumerate(d for d in docs if len(d) < 300)][:n]
    got, _, _, _ = run(codec, recs)
    assert got["doc"].shape == (n,) and got["kind"].shape == (n, 16) and (got["doc"] == J.OK).sum() >= n // 2


def test_member_name_at_every_chunk_phase(codec):
    """The matched name at each of the 16 byte phases of a staged 16-byte chunk."""
    recs, at = [], 0
    for rep in range(3):
        for phase in range(16):
            for pad in range(16):
                rec = wrap(b" " * pad + b'{"q":0,"a":{"b":"val%d"}}' % phase, phase)
                if (at + rec.index(b'"a"') + 1) % 16 == phase:
                    break
            recs.append(rec)
            at += len(rec)
    got, data, off, _ = run(codec, recs)
    raw = data.tobytes()
    assert {(raw.index(b'"a"', int(off[i])) + 1) % 16 for i in range(len(recs))} == set(range(16))
    p = J.HAND_PATHS.index("a.b")
    assert (got["kind"][:, p] == J.STR).all() and (got["len"][:, p] == np.array([4 + (i % 16 > 9) for i in range(48)])).all()


@pytest.mark.parametrize("lead", [0, 11])
def test_member_name_across_window_edges(codec, lead):
    """Tiles of more than one window, their record sizes sweeping the window's edge over the bytes
    of a matched name and of its value: the record that straddles the edge waits for the next
    window, the one before it ends with the window."""
    recs = []
    for t in range(16):
        fill = b"w" * (200 + t)
        for j in range(64):
            recs.append(wrap(b'{"f":"%s","a":{"b":"v%d","e":[%d]},"s":"\\u0041"}' % (fill, j, t), j))
    got, data, off, _ = run(codec, recs, lead=lead)
    p = J.HAND_PATHS.index("a.e")
    assert (got["kind"][1:, p] == J.ARR).all() and (got["doc"][1:] == J.OK).all()
    sizes = np.diff(off.astype(np.int64))[1:].reshape(16, 64).sum(axis=1)
    assert (sizes > WIN).all()  # every tile takes more than one window
    edges = {int(WIN - (off[1 + 64 * t + np.searchsorted(off[1 + 64 * t:] - off[1 + 64 * t], WIN) - 1] - off[1 + 64 * t])) % 16
             for t in range(16)}
    assert len(edges) >= 6, edges


def test_tiles_of_several_windows_and_long_records(codec):
    """Tiles whose 64 records need several windows; documents just under and over the window size
    (the longest staged one and the first read from HBM); one far longer than the window."""
    recs = []
    for i in range(64 * 2 + 9):
        fill = b"y" * (300 + 41 * (i % 9))
        recs.append(wrap(b'{"f":"%s","a":{"b":{"c":{"d":%d}}},"s":"x"}' % (fill, i), i))
    head = len(wrap(b"", 0)) - 2 - 2  # bytes of a record before its payload
    for size in (16000, WIN - 17, WIN - 16, WIN - 15, WIN, 17000, 60000):
        shell = b'{"f":"%s","a":{"b":{"c":{"d":-1}}},"s":"\\n"}'
        doc = shell % (b"z" * (size - len(shell % b"")))
        assert len(doc) == size
        recs.insert(70, wrap(doc, size))
    got, data, off, dec = run(codec, recs, lead=7)
    assert head > 0 and (got["doc"][1:] == J.OK).all()
    p = J.HAND_PATHS.index("a.b.c.d")
    assert (got["kind"][1:, p] == J.NUM).all() and (got["kind"][1:, J.HAND_PATHS.index("a")] == J.OBJ).all()
    long = np.nonzero(np.diff(off.astype(np.int64)) > 15000)[0]
    assert long.size == 7 and (got["kind"][long, J.HAND_PATHS.index("s")] == J.ESC).all()
    # bare documents of the same sizes: the document is the whole record
    docs = [bytes(data[int(off[i]) + int(dec["view_off"][i, 3]):][:int(dec["view_len"][i, 3])]) for i in range(60, 85)]
    got, _, _, _ = run(codec, docs, lead=2, decoded=False)
    assert (got["doc"][1:] == J.OK).all()


@pytest.mark.parametrize("view", [3, 4])
def test_random_records_of_mixed_kinds(codec, view):
    """3 000 random records: Acks, session events and error records are NOT_SELECTED; payloads
    (view 3) and headers (view 4, empty under SBE_FL_HEADERS_E100); a select mask."""
    recs = J.random_records(3000, 4242)
    sel = J.random_select(len(recs) + 1, 99)
    got, _, _, dec = run(codec, recs, lead=5, view=view, select=sel)
    tm = dec["status"] == T.ST_TM
    assert (got["doc"][~tm] == J.NOT_SELECTED).all() and (~tm).sum() >= 200
    assert (got["doc"][sel == 0] == J.NOT_SELECTED).all() and (sel == 0).sum() >= 50
    docs = np.bincount(got["doc"], minlength=5)
    assert all(docs[c] >= 20 for c in range(4)) and docs[J.STACK] >= 5, docs
    kinds = np.bincount(got["kind"].reshape(-1), minlength=9)
    assert all(kinds[k] >= 100 for k in range(1, 9)), kinds
    cut = tm & ((dec["flags"] & 0x4) != 0) & (sel != 0)
    assert cut.sum() >= 10 and (view != 4 or (got["doc"][cut] == J.EMPTY).all())


@pytest.mark.parametrize("table", [J.PATHS_1, ["s"], ["k.k.k.k"], J.HAND_PATHS, ["a.b.c.d", "m.y.z", "a.b.c"],
                                   ["p%d.a.b.c" % i for i in range(16)]],
                         ids=["1-depth2", "1-depth1", "1-depth4", "16-mixed", "3-deep", "16-depth4"])
def test_tables(codec, table):
    docs = J.random_docs(1500, 31) + J.hand_docs()
    got, _, _, _ = run(codec, docs, table=table, decoded=False)
    assert got["kind"].shape == (len(docs), len(table))
    if table[0][0] != "p":
        assert (got["kind"] != 0).sum() >= 50


def test_bare_random_documents_with_select(codec):
    docs = J.random_docs(3000, 5)
    sel = J.random_select(len(docs), 6, p=0.2)
    got, _, _, _ = run(codec, docs, decoded=False, select=sel)
    assert (got["doc"][sel == 0] == J.NOT_SELECTED).all() and (got["doc"][sel != 0] != J.NOT_SELECTED).all()
    assert (got["doc"] == J.STACK).sum() >= 10 and (got["doc"] == J.EMPTY).sum() >= 20


def test_repeat_call_and_empty_batch(codec):
    recs = J.random_records(64 * 3 + 5, 41)
    data, off = T.pack_records(recs)
    exp = J.ref_extract(data, off, T.oracle_decode(data, off, T.DEC_PARSE), J.HAND_PATHS)
    d, ro = to_dev(data, torch.uint8), to_dev(off, torch.int64)
    dec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE)
    first = codec.extract_json(d, ro, dec, J.HAND_PATHS)
    torch.cuda.synchronize()
    a = first.numpy()
    again = codec.extract_json(d, ro, dec, J.HAND_PATHS, out=first)  # the same buffers
    torch.cuda.synchronize()
    J.same(a, exp, "first", data, off)
    J.same(again.numpy(), exp, "again", data, off)
    # n == 0: SBE_OK, no launch, nothing written
    def poisoned(w, t):
        raw = torch.full((4 * max(w, 1) * (4 if t == I32 else 1),), 0x5A, dtype=U8, device="cuda").view(t)
        return raw.view(4, w) if w else raw

    out = codec.JsonFields(*(poisoned(w, t) for w, t in ((0, U8), (0, U8), (16, U8), (16, I32), (16, I32))))
    none = codec.extract_json(d, ro[:1], None, J.HAND_PATHS, out=out)
    torch.cuda.synchronize()
    assert none.doc.numel() == 0 and bool((out.doc == 0x5A).all()) and bool((out.kind == 0x5A).all())
    assert bool((out.off.view(U8) == 0x5A).all()) and bool((out.len.view(U8) == 0x5A).all())


@pytest.mark.parametrize("n_paths,decoded", [(16, True), (9, True), (1, False), (3, False)])
def test_outputs_between_poisoned_bands(codec, n_paths, decoded):
    """Every element i < n of the five arrays is written and nothing else: outputs at their
    minimal alignment between guard bands, one run per poison."""
    table = (J.HAND_PATHS + J.HAND_PATHS)[3:3 + n_paths]
    recs = J.random_records(64 * 5 + 3, 8) if decoded else J.random_docs(64 * 5 + 3, 8)
    data, off = T.pack_records(recs)
    n = len(recs)
    exp_dec = T.oracle_decode(data, off, T.DEC_PARSE) if decoded else None
    exp = J.ref_extract(data, off, exp_dec, table)
    d_in, r_in = C.placed(data, 1), C.placed(off, 8)
    dec = dec_inputs(codec, exp_dec) if decoded else None

    def once(r):
        out = codec.JsonFields(r.buf("doc", n, U8), r.buf("root_kind", n, U8), r.buf("kind", n * n_paths, U8).view(n, n_paths),
                               r.buf("off", n * n_paths, I32).view(n, n_paths), r.buf("len", n * n_paths, I32).view(n, n_paths))
        codec.extract_json(d_in, r_in, dec, table, out=out)
        torch.cuda.synchronize()
        for k in J.KEYS:
            r.expect(k, exp[k])

    C.twice(once)


def test_runs_on_the_callers_stream(codec):
    n = 1000
    data, off = T.pack_records(J.random_records(n, 55))
    exp_dec = T.oracle_decode(data, off, T.DEC_PARSE)
    exp = J.ref_extract(data, off, exp_dec, J.HAND_PATHS)
    d_in, r_in, dec = dev(data), dev(off), dec_inputs(codec, exp_dec)
    table = codec.json_path_table(J.HAND_PATHS)
    bufs = dict(doc=torch.empty(n, dtype=U8, device="cuda"), root_kind=torch.empty(n, dtype=U8, device="cuda"),
                kind=torch.empty((n, 16), dtype=U8, device="cuda"), off=torch.empty((n, 16), dtype=I32, device="cuda"),
                len=torch.empty((n, 16), dtype=I32, device="cuda"))
    out = codec.JsonFields(**bufs)

    def verify(host, poison):
        for key in J.KEYS:
            _need(host, poison, key, exp[key])

    on_side_stream(bufs, lambda s: codec.extract_json(d_in, r_in, dec, table, out=out, stream=s), verify)


def test_einval_writes_nothing(codec):
    recs = [wrap(d, i) for i, d in enumerate(J.hand_docs()[:40])]
    data, off = T.pack_records(recs)
    d, ro = to_dev(data, torch.uint8), to_dev(off, torch.int64)
    dec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE)
    n, P_ = len(recs), 16
    bufs = {f: torch.full(((n + 70) * P_ * {"uint8": 1, "uint32": 4}[t] + 8,), 0xA5, dtype=torch.uint8, device="cuda")
            for f, t in codec._JSON_KEYS}
    roff = torch.zeros(8 * (n + 1) + 8, dtype=torch.uint8, device="cuda")
    roff[4: 4 + 8 * (n + 1)] = ro.view(torch.uint8)
    vo_mis = torch.zeros(dec.view_off.numel() * 4 + 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(table=J.HAND_PATHS, **kw):
        a = dict(data=d.data_ptr(), rec_off=ro.data_ptr(), status=dec.status.data_ptr(), flags=dec.flags.data_ptr(),
                 view_off=dec.view_off.data_ptr(), view_len=dec.view_len.data_ptr(), dec=True, out=True, paths=True,
                 view=3, select=None, **{f: b.data_ptr() for f, b in bufs.items()})
        a.update(kw)
        P, depth, names, name_off = J.path_table(table)
        ps = codec._JsonPaths(P, depth.ctypes.data, names.ctypes.data, name_off.ctypes.data)
        dd = codec._Decoded(a["status"], a["flags"], dec.hdr.data_ptr(), dec.ts.data_ptr(), a["view_off"], a["view_len"], None)
        oo = codec._JsonOut(*(a[f] for f, _ in codec._JSON_KEYS))
        rc = codec.lib().sbe_json_extract_batch(a["data"], a["rec_off"], n, ctypes.byref(dd) if a["dec"] else None, a["view"],
                                                a["select"], ctypes.byref(ps) if a["paths"] else None,
                                                ctypes.byref(oo) if a["out"] else None, None, 0, None)
        torch.cuda.synchronize()
        return rc

    cases = [dict(data=None), dict(rec_off=None), dict(status=None), dict(flags=None), dict(view_off=None),
             dict(view_len=None), dict(out=False), dict(paths=False), dict(view=0), dict(view=2), dict(view=5),
             dict(dec=False), dict(dec=False, view=4), dict(rec_off=roff.data_ptr() + 4), dict(view_off=vo_mis.data_ptr() + 1),
             dict(view_len=vo_mis.data_ptr() + 2), dict(off=bufs["off"].data_ptr() + 2), dict(len=bufs["len"].data_ptr() + 1)]
    cases += [{f: None} for f, _ in codec._JSON_KEYS]
    cases += [dict(table=["a", "a"]), dict(table=["a.b.c.d.e"]), dict(table=[[b""]]), dict(table=["p%d" % i for i in range(17)])]
    for c in cases:
        assert call(**c) == -1, c  # SBE_EINVAL
    for f, b in bufs.items():
        assert bool((b == 0xA5).all()), f
    assert call() == 0
    assert not bool((bufs["doc"][:n] == 0xA5).any()) and bool((bufs["doc"][n:] == 0xA5).all())


def _strings(got, data, off, p):
    raw = data.tobytes()
    res = []
    for i in range(got["doc"].size):
        if got["kind"][i, p] not in (J.STR, J.ESC):
            res.append(None)
            continue
        b = int(off[i]) + int(got["off"][i, p])
        tok = raw[b:b + int(got["len"][i, p])]
        res.append(tok if got["kind"][i, p] == J.STR else J.unescape(tok))
    return res


def test_round_trip_edge_orders(codec):
    """2 000 edge Orders (escapes, non-ASCII, controls, NUL, empty client_order_uuid) through
    sbe_publish_orders_batch, a parse-mode decode and the nine order-id paths: the decoded
    client_order_id and uuid are each Order's client_order_uuid."""
    n = 2000
    fields, cid, ts, q = T.order_batch(n, 0xEDE, hard=True)
    for i in range(0, n, 37):
        fields[i][0] = b""
    z = np.zeros(n)
    b = P.Batch(fields, cid, ts, q, [b"LIMIT"] * n, [b"GTC"] * n, z, z, np.zeros(n, np.uint8))
    out, out_off, status, _ = P.run_device(codec, b, b"orders", None, 7, 1, True, 3, 4, validate=False)
    keep = np.nonzero(status == 0)[0]
    assert keep.size >= n - 20, np.bincount(status)
    data = out[: int(out_off[-1])]
    got, exp, dec = extract(codec, data, out_off, J.ORDER_ID_PATHS)
    J.same(got, exp, "published", data, out_off)
    assert (got["doc"][keep] == J.OK).all() and (dec["status"][keep] == T.ST_TM).all()
    kinds = got["kind"][keep]
    assert (kinds[:, [0, 1, 4]] == J.OBJ).all() and (kinds[:, [2, 3, 6, 7]] == J.MISSING).all()
    coid, uuid = _strings(got, data, out_off, 5), _strings(got, data, out_off, 8)
    escaped = lossy = 0
    seen = dict(quote=0, control=0, nul=0, non_ascii=0, empty=0)
    for i in keep:
        want = fields[i][0]
        try:
            want.decode("utf-8")
        except UnicodeDecodeError as e:
            # jsoncpp's writer does not keep an ill-formed UTF-8 sequence (valueToQuotedString reads code
            # points): such a uuid does not come back from Order::to_json's text under any reader.  What
            # does hold: everything before the first ill-formed byte comes back, and both members carry
            # the same text.  The ranges of these records are also held to the restatement above.
            assert coid[i] is not None and coid[i] == uuid[i] and coid[i].startswith(want[: e.start]), (i, want, coid[i])
            lossy += 1
            continue
        assert coid[i] == want and uuid[i] == want, (i, want, coid[i], uuid[i])
        escaped += got["kind"][i, 5] == J.ESC
        seen["quote"] += b'"' in want or b"\\" in want
        seen["control"] += any(0 < c < 32 for c in want)
        seen["nul"] += 0 in want
        seen["non_ascii"] += any(c >= 128 for c in want)
        seen["empty"] += want == b""
    assert escaped >= 100 and all(v >= 20 for v in seen.values()), (escaped, seen)
    assert lossy <= 380, lossy  # the generator draws 369 ill-formed uuids for this seed, before the 55 emptied ones


def test_fixed256_orders(codec):
    """20 000 fixed-256 Orders, the nine order-id paths."""
    n = 20000
    arena, L, ts = T.fixed256_orders(n)
    data, off, _ = T.oracle_encode(arena, L, ts)
    got, exp, _ = extract(codec, data, off, J.ORDER_ID_PATHS)
    J.same(got, exp, "fixed256")
    assert (got["doc"] == J.OK).all() and (got["root_kind"] == J.OBJ).all()
    assert (got["kind"] == J.MISSING).all()  # these payloads are flat: no "message", no "uuid"
    got, exp, _ = extract(codec, data, off, ["client_order_id", "message.message", "qty"])
    J.same(got, exp, "fixed256 flat")
    assert (got["kind"] == [J.STR, J.MISSING, J.STR]).all() and (got["len"] == [21, 0, 9]).all()
