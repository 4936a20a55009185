"""CPU: the sequential models of delivery tracking (tests/delivery_lib.py) on hand cases, and the
properties of the generated sequences the GPU test relies on."""
import numpy as np

import delivery_lib as D
import inflight_lib as I
import jsonpaths_lib as J
import sbe_testlib as T

SEED = 6      # of the random sequence of tests/test_gpu_delivery.py
E2E_SEED = 21  # of its end-to-end batches


def test_same_id_three_times_then_once_more():
    t = D.Table()
    code, count, totals = t.note([b"m1", b"m1", None, b"m1"])
    assert list(code) == [D.DLV_NEW, D.DLV_AGAIN, D.DLV_NONE, D.DLV_AGAIN]
    assert list(count) == [2, 2, 0, 2] and list(totals) == [1, 2]
    code, count, totals = t.note([b"m1", b"m2"])
    assert list(code) == [D.DLV_AGAIN, D.DLV_NEW] and list(count) == [3, 0] and list(totals) == [1, 1]
    assert t.header(64) == {"capacity": 64, "live": 2, "used": 2, "answered": 0}
    t.reset_values()
    code, count, _ = t.note([b"m1"])  # membership stays, the count starts again
    assert list(code) == [D.DLV_AGAIN] and list(count) == [1]


def test_count_is_what_record_duplicate_delivery_returned_last():
    t, cb = D.Table(), D.Callback()
    ids = [b"a", b"b", b"a", b"a", b"b", b"a"]
    code, count, _ = t.note(ids)
    res = [cb.on_message(m, b"", b"", 0) for m in ids]
    assert [r["already_processed"] for r in res] == [c == D.DLV_AGAIN for c in code]
    last = {m: i for i, m in enumerate(ids)}
    for m, i in last.items():
        assert res[i]["redeliveries"] == count[i]
    assert cb.messages_received == 2


def test_long_and_empty_keys():
    t = D.Table()
    code, count, totals = t.note([b"", b"x" * 40, b"x" * 41, b""])
    assert list(code) == [D.DLV_NEW, D.DLV_NEW, D.DLV_LONG, D.DLV_AGAIN] and list(count) == [1, 0, 0, 1]
    assert list(D.Table(key_max=None).note([b"x" * 41])[0]) == [D.DLV_NEW]
    code, value, totals = t.lookup([b"x" * 41, b"nobody", None, b""])
    assert list(code) == [D.SENT_LONG, D.SENT_UNKNOWN, D.SENT_NONE, D.SENT_FIRST]
    assert list(value) == [0, 0, 0, 2] and list(totals) == [1, 0, 2]


def test_lookup_marks_on_first_sight():
    t = D.Table()
    t.remember([b"c1", b"c2"], np.array([10, 20], np.uint64))
    code, value, totals = t.lookup([b"c1", b"c1", b"c3"])
    assert list(code) == [D.SENT_FIRST, D.SENT_REPEAT, D.SENT_UNKNOWN]
    assert list(value) == [10, 0, 0] and list(totals) == [1, 1, 1]
    assert list(t.lookup([b"c1", b"c2"])[0]) == [D.SENT_REPEAT, D.SENT_FIRST]
    # remember reports an answered key as a duplicate and leaves it answered
    assert list(t.remember([b"c1"], np.array([99], np.uint64))) == [I.INF_DUPLICATE]
    assert list(t.lookup([b"c1"])[0]) == [D.SENT_REPEAT]
    t.rehash()
    assert list(t.lookup([b"c1"])[0]) == [D.SENT_REPEAT] and t.header(64)["answered"] == 2
    # an ack still matches and erases it
    code, base, _ = t.match([(T.ST_EG_ACK, b"c1", 500)])
    assert list(code) == [I.ACK_MATCHED] and list(base) == [10]
    assert t.header(64) == {"capacity": 64, "live": 1, "used": 2, "answered": 1}
    assert list(t.lookup([b"c1"])[0]) == [D.SENT_UNKNOWN]


def test_callback_hand_case():
    cb = D.Callback()
    cb.publish(b"c1", 100)
    cb.publish(b"c2", 110)
    r = cb.on_message(b"m1", b"c1", b"o1", 150)
    assert r == dict(already_processed=False, redeliveries=0, duplicate_client_order=False, was_sent=True,
                     latency_recorded=True, latency=50)
    r = cb.on_message(b"m1", b"c1", b"o1", 170)  # the same message again
    assert r["already_processed"] and r["redeliveries"] == 1 and not r["duplicate_client_order"] and not r["latency_recorded"]
    r = cb.on_message(b"m2", b"c1", b"o1", 180)  # another message for the same order
    assert not r["already_processed"] and r["duplicate_client_order"] and r["was_sent"] and not r["latency_recorded"]
    r = cb.on_message(b"", b"c9", b"", 190)  # an empty message id is never a redelivery
    assert not r["already_processed"] and not r["was_sent"] and not r["latency_recorded"]
    assert cb.on_message(b"", b"c9", b"", 191)["duplicate_client_order"]
    assert cb.on_message(b"m1", b"", b"", 200)["redeliveries"] == 2
    cb.clear_duplicate_tracking()
    assert cb.on_message(b"m1", b"", b"", 210)["redeliveries"] == 1
    assert cb.messages_received == 4 and cb.missing() == {b"c2"} and cb.extra() == {b"c9"}


def test_pack_ranges_and_the_clamp():
    buf, pos, ln = D.pack_ranges([b"ab", None, b"", b"xyz"])
    assert bytes(buf) == b"\xEE\xEE\xEEab\xEE\xEExyz" and int(pos[3]) + 3 == buf.size  # the last key ends the buffer
    assert D.keys_of(buf, pos, ln) == [b"ab", None, b"", b"xyz"]
    assert D.keys_of(buf, pos, ln, buf_bytes=9) == [b"ab", None, b"", b"xy"]
    assert D.keys_of(buf, [100], [5]) == [b""]  # a position past the buffer is the empty key


def test_key_rule_on_every_format():
    coid, oid = b"client-1", b"order-1"
    recs = [D.order_record(b"m%d" % j, f, coid, oid) for j, f in enumerate(D.FORMATS)]
    recs += [D.order_record(b"", "inner", coid, oid), T.ack_wire(b"a", b"t", b"c", 1), D.order_record(b"u", "inner", coid, oid)]
    select = np.ones(len(recs), np.uint8)
    select[-1] = 0
    data, off, dec, ids, keys = D.parsed(recs, select)
    for j, f in enumerate(D.FORMATS):
        mid, c, o = D.strings_of(data, keys, j)
        hc, ho = D.has_ids(f)
        assert (mid, c, o) == (b"m%d" % j, coid if hc else b"", oid if ho else b""), f
        assert (c, o) == J.ref_order_ids(D.payload(f, coid, oid)), f  # the reference's callback body itself
        assert (c, o) == J.order_ids_from_fields(ids, data, off, j), f
    k = {f: j for j, f in enumerate(D.FORMATS)}
    assert keys["coid_kind"][k["escaped"]] == J.ESC and keys["oid_kind"][k["escaped"]] == J.ESC
    assert keys["coid_kind"][k["esc_stop"]] == J.ESC and keys["oid_kind"][k["esc_stop"]] == J.STR
    assert keys["coid_kind"][k["non_string"]] == J.MISSING and keys["coid_len"][k["non_string"]] == D.NO_KEY
    n = len(D.FORMATS)
    assert keys["msg_len"][n] == D.NO_KEY and keys["selected"][n] == 1 and keys["coid_len"][n] == len(coid)
    assert list(keys["selected"][n + 1:]) == [0, 0] and keys["msg_len"][n + 2] == D.NO_KEY
    assert list(keys["totals"]) == [n + 1, 3]
    # the patch that makes an escaped id comparable
    buf, pos, ln = D.patch_escaped(data, keys)
    j = k["escaped"]
    assert int(pos[j]) >= data.size and bytes(buf[int(pos[j]):][:int(ln[j])]) == coid
    assert bytes(buf[: data.size]) == bytes(data)


def test_random_sequence_holds_every_class():
    pool, ops = D.random_ops(SEED)
    assert len(ops) == 20 and {len(k) for k in pool} >= set(I.EDGE_LENS)
    t = D.Table()
    codes = {"note": set(), "lookup": set()}
    for op in ops:
        if op[0] == "remember":
            t.remember(op[1], op[2])
        elif op[0] in ("note", "lookup"):
            assert len(op[1]) <= 300 and None in op[1]
            codes[op[0]] |= set(getattr(t, op[0])(op[1])[0])
        else:
            getattr(t, {"reset": "reset_values", "rehash": "rehash"}[op[0]])()
        assert t.used <= 1024 - 8
    assert codes["note"] == {D.DLV_NONE, D.DLV_NEW, D.DLV_AGAIN, D.DLV_LONG}
    assert codes["lookup"] == {D.SENT_NONE, D.SENT_UNKNOWN, D.SENT_FIRST, D.SENT_REPEAT, D.SENT_LONG}
    assert all(t.seen[k] >= 5 for k in ("again_in_call", "again_live", "first_then_repeat", "repeat_across", "long",
                                        "count5")), t.seen


def e2e_batches():
    """The two batches of the end-to-end GPU test and the ids the publisher sent."""
    coids = D.client_ids(260, E2E_SEED)
    first, sel1 = D.delivery_batch(E2E_SEED, 300, coids)
    kept = [r for r in first if T.oracle_decode(*T.pack_records([r]), T.DEC_PARSE)["status"][0] == T.ST_TM]
    second, sel2 = D.delivery_batch(E2E_SEED + 1, 300, coids, first_msg=1000, prior=kept)
    return coids[:200], ((first, sel1), (second, sel2))


def test_end_to_end_batches_hold_every_class():
    sent, batches = e2e_batches()
    cb = D.Callback()
    msgs, clients, sends = D.Table(), D.Table(), D.Table()
    for c in sent:
        cb.publish(c, 1000)
    sends.remember(sent, np.full(len(sent), 1000, np.uint64))
    seen = dict(esc=0, long_coid=0, long_msg=0, redelivered=0, dup_order=0, latency=0, count5=0, unselected=0, no_msg=0)
    for b, (recs, select) in enumerate(batches):
        data, off, dec, ids, keys = D.parsed(recs, select)
        assert 250 <= len(recs) <= 300
        buf, cpos, clen = D.patch_escaped(data, keys)
        mk = D.keys_of(buf, keys["msg_pos"], keys["msg_len"])
        ck = D.keys_of(buf, cpos, clen)
        mcode, mcount, _ = msgs.note(mk)
        ccode, _, _ = clients.note(ck)
        scode, sval, _ = sends.lookup(ck)
        for i in range(len(recs)):
            if not keys["selected"][i]:
                seen["unselected"] += 1
                assert mk[i] is None and ck[i] is None
                continue
            mid, c, o = D.strings_of(data, keys, i)
            assert (mk[i] or b"", ck[i] or b"") == (mid, c)
            r = cb.on_message(mid, c, o, 5000 + b)
            seen["esc"] += keys["coid_kind"][i] == J.ESC
            seen["long_msg"] += mcode[i] == D.DLV_LONG
            seen["long_coid"] += ccode[i] == D.DLV_LONG
            seen["no_msg"] += mcode[i] == D.DLV_NONE
            seen["count5"] += r["redeliveries"] >= D.RECONNECT_THRESHOLD
            if mcode[i] != D.DLV_LONG:  # the table tells what the callback tells
                assert r["already_processed"] == (mcode[i] == D.DLV_AGAIN)
                seen["redelivered"] += r["already_processed"]
            if mcode[i] != D.DLV_LONG and ccode[i] != D.DLV_LONG:
                assert r["duplicate_client_order"] == (ccode[i] == D.DLV_AGAIN and mcode[i] != D.DLV_AGAIN)
                assert r["was_sent"] == (scode[i] in (D.SENT_FIRST, D.SENT_REPEAT))
                assert r["latency_recorded"] == (scode[i] == D.SENT_FIRST)
                assert not r["latency_recorded"] or r["latency"] == 5000 + b - int(sval[i])
                seen["dup_order"] += r["duplicate_client_order"]
                seen["latency"] += r["latency_recorded"]
        last = {m: i for i, m in enumerate(mk) if m is not None and mcode[i] == D.DLV_AGAIN}
        assert all(int(mcount[i]) == cb.duplicate_delivery_counts[m] for m, i in last.items())
    assert all(v >= 3 for v in seen.values()), seen
    assert msgs.seen["again_live"] >= 20 and msgs.seen["again_in_call"] >= 20  # across the batches and inside one
    assert sends.seen["repeat_across"] >= 5 and sends.seen["first_then_repeat"] >= 5
