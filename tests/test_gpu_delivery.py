"""GPU: delivery tracking (sbe_inflight_note_keys, sbe_inflight_lookup_keys,
sbe_inflight_reset_values, sbe_delivery_keys) against the sequential models of
tests/delivery_lib.py.  Every comparison is exact, and the header words of a table are checked
after every step."""
import numpy as np
import pytest
import torch

import contract_lib as C
import delivery_lib as D
import inflight_lib as I
import jsonpaths_lib as J
import sbe_testlib as T
from test_delivery_lib import SEED, e2e_batches
from test_gpu_contract import DEC_KEYS, dec_inputs, dev, u
from test_gpu_inflight import acks_for, check_match, match, remember, same

pytestmark = pytest.mark.gpu

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
TAGS = [1, 0]


def ranges(keys, buf_bytes=None):
    buf, pos, ln = D.pack_ranges(keys)
    return dev(buf if buf.size else np.zeros(1, np.uint8)), dev(pos), dev(ln), int(buf.size) if buf_bytes is None else buf_bytes


def note(tbl, keys):
    b, p, l, nb = ranges(keys)
    return tbl.note_keys(b, p, l, buf_bytes=nb).numpy()


def lookup(tbl, keys):
    b, p, l, nb = ranges(keys)
    return tbl.lookup_keys(b, p, l, buf_bytes=nb).numpy()


def check(got, exp, names, what):
    for k, e in zip(names, exp):
        same(got[k], e, f"{what}: {k}")


NOTE, LOOKUP = ("code", "count", "totals"), ("code", "value", "totals")


def check_header(tbl, model):
    assert tbl.stats_ex() == model.header(tbl.capacity)
    assert tbl.stats() == {k: v for k, v in model.header(tbl.capacity).items() if k != "answered"}


# ------------------------------------------------------------------------------------------
# hand cases
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag_bits", TAGS)
def test_hand_note(codec, tag_bits):
    tbl, m = codec.Inflight(64, "cuda", tag_bits), D.Table()
    got = note(tbl, [b"m1", b"m1", None, b"m1"])
    assert list(got["code"]) == [D.DLV_NEW, D.DLV_AGAIN, D.DLV_NONE, D.DLV_AGAIN] and list(got["count"]) == [2, 2, 0, 2]
    check(got, m.note([b"m1", b"m1", None, b"m1"]), NOTE, "first call")
    check_header(tbl, m)
    got = note(tbl, [b"m1", b"m2"])
    assert list(got["code"]) == [D.DLV_AGAIN, D.DLV_NEW] and list(got["count"]) == [3, 0] and list(got["totals"]) == [1, 1]
    check(got, m.note([b"m1", b"m2"]), NOTE, "second call")
    check_header(tbl, m)
    tbl.reset_values()  # the counts go, membership stays
    m.reset_values()
    check_header(tbl, m)
    got = note(tbl, [b"m2", b"m1", b"m3", b"m1"])
    assert list(got["code"]) == [D.DLV_AGAIN, D.DLV_AGAIN, D.DLV_NEW, D.DLV_AGAIN] and list(got["count"]) == [1, 2, 0, 2]
    check(got, m.note([b"m2", b"m1", b"m3", b"m1"]), NOTE, "after the reset")
    check_header(tbl, m)
    got = note(tbl, [b"", b"x" * 40, b"x" * 41, b""])  # emplace("") succeeds; 41 bytes are not stored
    assert list(got["code"]) == [D.DLV_NEW, D.DLV_NEW, D.DLV_LONG, D.DLV_AGAIN]
    check(got, m.note([b"", b"x" * 40, b"x" * 41, b""]), NOTE, "edge lengths")
    check_header(tbl, m)


@pytest.mark.parametrize("tag_bits", TAGS)
def test_hand_lookup(codec, tag_bits):
    tbl, m = codec.Inflight(64, "cuda", tag_bits), D.Table()
    ts = np.array([10, 20, 30], np.uint64)
    same(remember(tbl, [b"c1", b"c2", b"c3"], ts), m.remember([b"c1", b"c2", b"c3"], ts), "status")
    keys = [b"c1", b"c1", b"c4", None, b"z" * 41]
    got = lookup(tbl, keys)
    assert list(got["code"]) == [D.SENT_FIRST, D.SENT_REPEAT, D.SENT_UNKNOWN, D.SENT_NONE, D.SENT_LONG]
    assert list(got["value"]) == [10, 0, 0, 0, 0] and list(got["totals"]) == [1, 1, 2]
    check(got, m.lookup(keys), LOOKUP, "first call")
    check_header(tbl, m)
    got = lookup(tbl, [b"c2", b"c1"])  # answered in an earlier call
    assert list(got["code"]) == [D.SENT_FIRST, D.SENT_REPEAT] and list(got["value"]) == [20, 0]
    check(got, m.lookup([b"c2", b"c1"]), LOOKUP, "second call")
    check_header(tbl, m)
    # remember of an answered key is a duplicate, and the key stays answered
    st = remember(tbl, [b"c1", b"c5"], [99, 50])
    assert list(st) == [I.INF_DUPLICATE, I.INF_INSERTED]
    same(st, m.remember([b"c1", b"c5"], np.array([99, 50], np.uint64)), "status")
    check(lookup(tbl, [b"c1", b"c5"]), m.lookup([b"c1", b"c5"]), LOOKUP, "after remember")
    check_header(tbl, m)
    # rehash carries the mark
    tbl = tbl.rehash(128, tag_bits=tag_bits)
    m.rehash()
    check_header(tbl, m)
    got = lookup(tbl, [b"c1", b"c3"])
    assert list(got["code"]) == [D.SENT_REPEAT, D.SENT_FIRST] and list(got["value"]) == [0, 30]
    check(got, m.lookup([b"c1", b"c3"]), LOOKUP, "after rehash")
    check_header(tbl, m)
    # an ack of an answered key still matches; `answered` drops with it
    got, acks = match(codec, tbl, acks_for([b"c1", b"c9"]))
    exp = m.match(acks)
    assert list(exp[0]) == [I.ACK_MATCHED, I.ACK_UNMATCHED] and int(exp[1][0]) == 10
    check_match(got, exp)
    check_header(tbl, m)
    assert m.header(128) == {"capacity": 128, "live": 3, "used": 4, "answered": 3}
    check(lookup(tbl, [b"c1"]), m.lookup([b"c1"]), LOOKUP, "after the ack")
    # a remembered key counts on from its send time
    check(note(tbl, [b"c2", b"c2"]), m.note([b"c2", b"c2"]), NOTE, "note on a sent key")
    assert m.inflight[b"c2"] == 22
    check_header(tbl, m)


def test_a_table_without_a_header_holds_nothing_and_has_no_room(codec):
    tbl = codec.Inflight(64, "cuda")
    tbl.table.zero_()  # not a table sbe_inflight_init made
    keys = [b"a", None, b"x" * 41, b"a"]
    got = note(tbl, keys)
    assert list(got["code"]) == [D.DLV_FULL, D.DLV_NONE, D.DLV_LONG, D.DLV_FULL]
    assert list(got["count"]) == [0] * 4 and list(got["totals"]) == [0, 0]
    got = lookup(tbl, keys)
    assert list(got["code"]) == [D.SENT_UNKNOWN, D.SENT_NONE, D.SENT_LONG, D.SENT_UNKNOWN]
    assert list(got["value"]) == [0] * 4 and list(got["totals"]) == [0, 0, 3]
    tbl.reset_values()
    assert int(tbl.table.count_nonzero()) == 0  # left untouched


# ------------------------------------------------------------------------------------------
# sizes: none, partial and several workgroups; small tables force long chains that wrap
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag_bits", TAGS)
@pytest.mark.parametrize("capacity", [64, 128, 1024])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sizes(codec, n, capacity, tag_bits):
    rng = np.random.default_rng(1000 * n + capacity)
    distinct = max(1, min(n, capacity - 8))  # every key comes from this pool: used + new keys <= capacity - 8
    pool = I.key_pool(distinct + 12, n + 1)[:distinct]
    pick = lambda: [None if rng.integers(0, 9) == 0 else pool[i] for i in rng.integers(0, len(pool), n)]  # noqa: E731
    tbl, m = codec.Inflight(capacity, "cuda", tag_bits), D.Table()
    sent = [k for k in pool[::2] if len(k) <= D.KEY_MAX]
    ts = rng.integers(1, 2 ** 63, len(sent), dtype=np.uint64)
    same(remember(tbl, sent, ts), m.remember(sent, ts), "status")
    for step in range(2):
        keys = pick()
        check(lookup(tbl, keys), m.lookup(keys), LOOKUP, f"lookup {step}")
        check_header(tbl, m)
        keys = pick()
        check(note(tbl, keys), m.note(keys), NOTE, f"note {step}")
        check_header(tbl, m)
    assert m.used <= capacity - 8
    if n == 257 and capacity == 64:
        assert m.used >= 45  # the chains of a table this full are long and wrap around its end


# ------------------------------------------------------------------------------------------
# keys: edge lengths, families, the clamp
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag_bits", TAGS)
def test_keys_that_differ_in_one_place_are_distinct(codec, tag_bits):
    keys = [b"a", b"a\0", b"a\0\0", b"b", b"", b"\0", b"x" * 39 + b"y", b"x" * 40, b"x" * 39, b"x" * 38 + b"\0",
            b"pub_1760000000000000000", b"pub_1760000000000000001", b"pub_176000000000000000"]
    tbl, m = codec.Inflight(64, "cuda", tag_bits), D.Table()
    got = note(tbl, keys)
    assert list(got["code"]) == [D.DLV_NEW] * len(keys) and list(got["totals"]) == [len(keys), 0]
    check(got, m.note(keys), NOTE, "note")
    probe = list(reversed(keys)) + [b"a\0\0\0", b"x" * 38, b"x" * 41, b"pub_17600000000000000"]
    got = lookup(tbl, probe)
    assert list(got["code"]) == [D.SENT_FIRST] * len(keys) + [D.SENT_UNKNOWN] * 2 + [D.SENT_LONG, D.SENT_UNKNOWN]
    assert list(got["value"][: len(keys)]) == [1] * len(keys)
    check(got, m.lookup(probe), LOOKUP, "lookup")
    check_header(tbl, m)


@pytest.mark.parametrize("tag_bits", TAGS)
def test_ranges_are_clamped_into_the_buffer(codec, tag_bits):
    """The last key ends exactly at buf_bytes, which ends the tensor; ranges that reach past
    buf_bytes are cut there, a position past it is the empty key; nothing behind it is read."""
    keys = [b"first", b"second", b"x" * 40]
    buf, pos, ln = D.pack_ranges(keys)
    nb = int(buf.size)
    assert int(pos[2]) + 40 == nb
    pos = np.concatenate([pos, np.array([pos[1], pos[2] + 1, nb - 2, nb, nb + 100, 2 ** 63], np.uint64)])
    ln = np.concatenate([ln, np.array([nb, 40, 0xFFFFFFFE, 5, 5, 5], np.uint32)])
    tbl, m = codec.Inflight(64, "cuda", tag_bits), D.Table()
    model_keys = D.keys_of(buf, pos, ln)
    assert model_keys[3:] == [bytes(buf[int(pos[1]):]), b"x" * 39, b"xx", b"", b"", b""]
    got = tbl.note_keys(dev(buf), dev(pos), dev(ln)).numpy()
    assert list(got["code"]) == [D.DLV_NEW] * 3 + [D.DLV_LONG, D.DLV_NEW, D.DLV_NEW, D.DLV_NEW, D.DLV_AGAIN, D.DLV_AGAIN]
    check(got, m.note(model_keys), NOTE, "note")
    # a shorter buf_bytes over the same tensor: the bytes behind it are not part of any key
    cut = nb - 10
    big = dev(np.concatenate([buf, np.full(64, 0x78, np.uint8)]))  # 'x' bytes behind the buffer
    model_keys = D.keys_of(buf, pos, ln, buf_bytes=cut)
    assert model_keys[2] == b"x" * 30
    got = tbl.lookup_keys(big, dev(pos), dev(ln), buf_bytes=cut).numpy()
    check(got, m.lookup(model_keys), LOOKUP, "lookup")
    got = tbl.note_keys(big, dev(pos), dev(ln), buf_bytes=cut).numpy()
    check(got, m.note(model_keys), NOTE, "note, cut")
    check_header(tbl, m)


# ------------------------------------------------------------------------------------------
# a random sequence of every operation on one shared table
# ------------------------------------------------------------------------------------------
def run_ops(codec, tbl, ops, model):
    outs = []
    for c, op in enumerate(ops):
        if op[0] == "remember":
            got = remember(tbl, op[1], op[2])
            same(got, model.remember(op[1], op[2]), f"call {c}: status")
            outs.append(got)
        elif op[0] in ("note", "lookup"):
            got = (note if op[0] == "note" else lookup)(tbl, op[1])
            names = NOTE if op[0] == "note" else LOOKUP
            check(got, getattr(model, op[0])(op[1]), names, f"call {c} ({op[0]})")
            outs.extend(got[k] for k in names)
        elif op[0] == "reset":
            tbl.reset_values()
            model.reset_values()
        else:
            tbl = tbl.rehash(tbl.capacity)
            model.rehash()
        st = tbl.stats_ex()
        assert st == model.header(tbl.capacity), (c, op[0])
        outs.append(np.array(list(st.values())))
    return outs


def test_random_sequence(codec):
    pool, ops = D.random_ops(SEED)  # tests/test_delivery_lib.py checks what this sequence holds
    runs = [run_ops(codec, codec.Inflight(1024, "cuda", tag_bits), ops, D.Table()) for tag_bits in TAGS]
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------
# the call contract (tests/contract_lib.py)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 257])
def test_key_calls_write_their_outputs_only(codec, n):
    rng = np.random.default_rng(70 + n)
    pool = I.key_pool(100, 70 + n)
    sent = [k for k in pool[:60] if len(k) <= D.KEY_MAX]
    keys = [[None if rng.integers(0, 7) == 0 else pool[i] for i in rng.integers(0, len(pool), n)] for _ in range(2)]
    model = D.Table()
    model.remember(sent, None, 77)
    exp_note, exp_look = model.note(keys[0]), model.lookup(keys[1])
    header = model.header(256)
    if n > 1:
        assert len(set(exp_note[0])) == 4 and len(set(exp_look[0])) == 5
    host = [D.pack_ranges(k) for k in keys]
    placed = [(C.placed(b, 1), C.placed(p, 8), C.placed(l, 4)) for b, p, l in host]
    ws_bytes = int(codec.lib().sbe_inflight_workspace_size(n))
    arena, off, ln = (dev(a) for a in I.pack_keys(sent))

    def one(run):
        tbl = codec.Inflight(256, "cuda", 1, table=run.buf("table", codec.Inflight.table_bytes(256), U8, align=64))
        tbl.remember(arena, off, ln, ts_default=77)
        b, p, l = placed[0]
        tbl.note_keys(b, p, l, code=run.buf("code", n, U8), count=run.buf("count", n, I32), totals=run.buf("totals", 2, I64),
                      workspace=run.buf("workspace", ws_bytes, U8, align=4))
        b, p, l = placed[1]
        tbl.lookup_keys(b, p, l, code=run.buf("code2", n, U8), value=run.buf("value", n, I64),
                        totals=run.buf("totals2", 3, I64), workspace=run.buf("workspace2", ws_bytes, U8, align=4))
        torch.cuda.synchronize()
        for name, exp in zip(("code", "count", "totals", "code2", "value", "totals2"), exp_note + exp_look):
            run.expect(name, exp)
        assert tbl.stats_ex() == header
        for (b, p, l), h in zip(placed, host):
            for t, a in zip((b, p, l), h):
                assert np.array_equal(u(t).reshape(-1), a.reshape(-1))
    C.twice(one)


# ------------------------------------------------------------------------------------------
# sbe_delivery_keys
# ------------------------------------------------------------------------------------------
def device_keys(codec, data, off, exp_dec, select, oracle_descriptors=True):
    d, ro = dev(data), dev(off)
    dec = codec.Decoded(*(dev(exp_dec[k]) for k in DEC_KEYS)) if oracle_descriptors else codec.decode_batch(
        d, ro, mode=codec.DEC_PARSE_MESSAGE)
    sel = None if select is None else dev(select)
    ids = codec.extract_json(d, ro, dec, codec.ORDER_ID_PATHS, select=sel)
    return d, ro, dec, sel, ids


def check_keys(got, exp, what="keys"):
    for k in D.KEY_FIELDS + ("totals",):
        same(got[k], exp[k], f"{what}: {k}")


def test_delivery_keys_on_every_format(codec):
    coid, oid = b"client-1", b"order-1"
    recs = [b"\0" * 5] + [D.order_record(b"m%d" % j, f, coid, oid) for j, f in enumerate(D.FORMATS)]
    recs += [D.order_record(b"", "inner", coid, oid), T.ack_wire(b"a", b"t", b"c", 1), D.order_record(b"u", "inner", coid, oid)]
    select = np.ones(len(recs), np.uint8)
    select[-1] = 0
    data, off, dec, ids, exp = D.parsed(recs, select)
    d, ro, ddec, sel, dids = device_keys(codec, data, off, dec, select)
    J.same(dids.numpy(), ids, "extract", data, off)
    got = codec.delivery_keys(ro, ddec, dids, select=sel).numpy()
    check_keys(got, exp)
    k = 1 + D.FORMATS.index("esc_stop")  # the escaped id at path 2 stopped the fall-through to order_details
    assert got["coid_kind"][k] == J.ESC and D.strings_of(data, got, k)[1] == coid
    assert list(got["totals"]) == [len(D.FORMATS) + 1, 3]
    # select == NULL: every TopicMessage
    exp_all = D.expected_keys(off, dec, None, J.ref_extract(data, off, dec, J.ORDER_ID_PATHS))
    assert exp_all["selected"][-1] == 1
    check_keys(codec.delivery_keys(ro, ddec, codec.extract_json(d, ro, ddec, codec.ORDER_ID_PATHS)).numpy(), exp_all, "no mask")


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 600])
def test_delivery_keys_on_generated_batches(codec, n):
    recs, select = D.delivery_batch(50 + n, n, D.client_ids(40, 3))
    data, off, dec, ids, exp = D.parsed(recs, select)
    if n >= 255:
        assert exp["totals"][1] > 0 and 0 < exp["totals"][0] < n
    pad = data if data.size else np.zeros(16, np.uint8)
    for oracle in (True, False):
        d, ro, ddec, sel, dids = device_keys(codec, pad, off, dec, select, oracle)
        check_keys(codec.delivery_keys(ro, ddec, dids, select=sel).numpy(), exp, f"oracle={oracle}")


@pytest.mark.parametrize("n", [1, 257])
def test_delivery_keys_writes_its_outputs_only(codec, n):
    recs, select = D.delivery_batch(90 + n, n, D.client_ids(40, 3))
    data, off, dec, ids, exp = D.parsed(recs, select)
    ro, ddec, sel = C.placed(off, 8), dec_inputs(codec, dec), C.placed(select, 1)
    dids = codec.JsonFields(C.placed(ids["doc"], 1), C.placed(ids["root_kind"], 1), C.placed(ids["kind"], 1),
                            C.placed(ids["off"], 4), C.placed(ids["len"], 4))
    types = {"pos": I64, "len": I32}

    def one(run):
        out = codec.DeliveryKeys(*(run.buf(k, n, types.get(k[-3:], U8)) for k in D.KEY_FIELDS), run.buf("totals", 2, I64))
        codec.delivery_keys(ro, ddec, dids, select=sel, out=out)
        torch.cuda.synchronize()
        for k in D.KEY_FIELDS + ("totals",):
            run.expect(k, exp[k])
        assert np.array_equal(u(dids.kind), ids["kind"]) and np.array_equal(u(ro), off)
    C.twice(one)


# ------------------------------------------------------------------------------------------
# end to end: remember the sent ids; decode -> extract -> keys -> note, note, lookup
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag_bits", TAGS)
def test_end_to_end(codec, tag_bits):
    sent, batches = e2e_batches()  # tests/test_delivery_lib.py checks what these batches hold
    msgs, clients, sends = (codec.Inflight(2048, "cuda", tag_bits) for _ in range(3))
    m_msgs, m_clients, m_sends = D.Table(), D.Table(), D.Table()
    ts = np.arange(1000, 1000 + len(sent), dtype=np.uint64)
    same(remember(sends, sent, ts), m_sends.remember(sent, ts), "status")
    cb = D.Callback()
    for c, t in zip(sent, ts):
        cb.publish(c, int(t))
    for b, (recs, select) in enumerate(batches):
        data, off, dec, ids, exp = D.parsed(recs, select)
        d, ro = dev(data), dev(off)
        ddec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE)
        sel = dev(select)
        dids = codec.extract_json(d, ro, ddec, codec.ORDER_ID_PATHS, select=sel)
        keys = codec.delivery_keys(ro, ddec, dids, select=sel)
        got = keys.numpy()
        check_keys(got, exp, f"batch {b}")
        # the escape path: decoded ids behind the batch, coid ranges patched
        assert got["totals"][1] > 0
        buf, cpos, clen = D.patch_escaped(data, got)
        dbuf, dcpos, dclen = dev(buf), dev(cpos), dev(clen)
        g_msg = msgs.note_keys(dbuf, keys.msg_pos, keys.msg_len, buf_bytes=int(data.size)).numpy()
        g_cli = clients.note_keys(dbuf, dcpos, dclen).numpy()
        g_snt = sends.lookup_keys(dbuf, dcpos, dclen).numpy()
        mk, ck = D.keys_of(buf, exp["msg_pos"], exp["msg_len"]), D.keys_of(buf, cpos, clen)
        check(g_msg, m_msgs.note(mk), NOTE, f"batch {b}: message ids")
        check(g_cli, m_clients.note(ck), NOTE, f"batch {b}: client ids")
        check(g_snt, m_sends.lookup(ck), LOOKUP, f"batch {b}: sent")
        for t, m in ((msgs, m_msgs), (clients, m_clients), (sends, m_sends)):
            check_header(t, m)
        # what the callback itself says, from the device's outputs
        now = 10_000 + b
        for i in np.nonzero(got["selected"])[0]:
            r = cb.on_message(*D.strings_of(data, got, i), now)
            if g_msg["code"][i] == D.DLV_LONG or g_cli["code"][i] == D.DLV_LONG:
                continue  # the host mirror's sets take these
            assert r["already_processed"] == (g_msg["code"][i] == D.DLV_AGAIN)
            assert r["duplicate_client_order"] == (g_cli["code"][i] == D.DLV_AGAIN and g_msg["code"][i] != D.DLV_AGAIN)
            assert r["was_sent"] == (g_snt["code"][i] in (D.SENT_FIRST, D.SENT_REPEAT))
            assert r["latency_recorded"] == (g_snt["code"][i] == D.SENT_FIRST)
            if r["latency_recorded"]:
                assert r["latency"] == now - int(g_snt["value"][i])
    assert m_msgs.seen["again_live"] >= 20 and m_sends.seen["repeat_across"] >= 5
