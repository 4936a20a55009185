"""GPU: sbe_classify_commits, the auto-commit decision of ClusterClient::handle_incoming_message
(src/cluster_client.cpp:1198-1303) on decoded batches.  Every output (cm, topic_src, topic_kind,
topic_off, topic_len, topic_idx, last, count) is compared bit-exactly with the restatement
tests/autocommit/commit_ref.cpp run over the oracle's decode of the same bytes (jsoncpp is absent:
parity with the library itself is unpinned, see test_autocommit_ref.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import autocommit_lib as A
import sbe_testlib as T
from test_autocommit_ref import RANDOM_N, RANDOM_SEED
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U64MAX = 2**64 - 1


def classify(codec, data, off, topics, lead_check=True):
    """GPU decode + classify of packed records; returns (got, expected, oracle decode)."""
    exp_dec = T.oracle_decode(data, off, T.DEC_PARSE)
    exp = A.ref_classify(data, off, exp_dec, topics)
    d = to_dev(data if data.size else np.zeros(16, np.uint8), torch.uint8)
    ro = to_dev(np.asarray(off, np.uint64), torch.int64)
    dec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE)
    plan = codec.classify_commits(d, ro, dec, topics)
    torch.cuda.synchronize()
    return plan.numpy(), exp, exp_dec


def assert_same(got, exp, data=None, off=None):
    for k in A.KEYS:
        assert got[k].shape == exp[k].shape, k
        bad = np.nonzero(got[k] != exp[k])[0]
        ctx = [] if data is None or k in ("last", "count") else \
            [data[int(off[i]):int(off[i + 1])].tobytes()[:160] for i in bad[:3]]
        assert bad.size == 0, (k, bad[:5], got[k][bad[:5]], exp[k][bad[:5]], ctx)


def run(codec, recs, topics=A.TOPICS, lead=None):
    data, off = T.pack_records(([b"\0" * lead] if lead is not None else []) + recs)
    got, exp, dec = classify(codec, data, off, topics)
    assert_same(got, exp, data, off)
    return got, data, off, dec


@pytest.mark.parametrize("lead", [0, 3, 9])
def test_hand_table(codec, lead):
    got, data, off, _ = run(codec, A.hand_records(), lead=lead)
    assert got["cm"][0] == A.NOT_PARSED  # the lead record
    A.check_hand(got, data, off, first=1)


def test_random_batch(codec):
    got, _, _, dec = run(codec, A.random_records(RANDOM_N, RANDOM_SEED), lead=5)
    cm = np.bincount(got["cm"], minlength=8)
    src = np.bincount(got["topic_src"], minlength=5)
    assert all(cm[c] >= 100 for c in (0, 2, 3, 4, 5, 6, 7)), cm
    assert all(src[s] >= 100 for s in (1, 2, 3, 4)), src


def test_needle_at_every_chunk_phase(codec):
    """The key at each of the 16 byte phases of a 16-byte chunk, in headers and in payloads."""
    recs, at = [], 0
    for rep in range(3):
        for phase in range(16):
            for kind in range(2):
                for pad in range(16):  # the padding that puts this record's key at the wanted phase
                    if kind == 0:
                        rec = T.tm_wire([b"t", b"X", b"m", A.P, b" " * pad + b'{"topic":"alpha"}'], phase)
                    else:
                        rec = T.tm_wire([b"t", b"X", b"m", b" " * pad + b'{"message":{"topic":"beta"}}', b"{}"], phase)
                    if (at + rec.index(b'"topic"') + 1) % 16 == phase:
                        break
                recs.append(rec)
                at += len(rec)
    got, data, off, _ = run(codec, recs)
    raw = data.tobytes()
    phases = set()
    for i in range(len(recs)):
        at = raw.index(b'"topic"', int(off[i]), int(off[i + 1])) + 1
        phases.add((at % 16, i % 2))
    assert len(phases) == 32
    assert (got["cm"] == A.COMMIT).all() and set(got["topic_idx"]) == {1, 2}


@pytest.mark.parametrize("lead", [0, 11])
def test_needle_at_tile_window_edges(codec, lead):
    """The key in the last record of one 64-record tile (its window's end) and the first of the
    next (its window's start), with the tiles' sizes sweeping the edge over every chunk phase."""
    recs = []
    for pair in range(16):
        for j in range(128):
            filler = b"x" * (pair + (j % 3))
            if j == 0 and pair == 0:  # the batch's first bytes shifted by `lead` without adding a record
                recs.append(T.tm_wire([b"t", b"X", b"m", b'{"a":"%s"}' % (b"x" * lead), b"{}"], j))
            elif j == 63:  # headers end the record: the key's value is the tile's last bytes
                recs.append(T.tm_wire([b"t", b"X", b"m", b'{"a":"%s"}' % filler, b'{"topic":"alpha"}'], j))
            elif j == 64:  # empty leading fields: the key sits right after the record's start
                recs.append(T.tm_wire([b"", b"", b"m", b'{"topic":"beta"}', b""], j))
            else:
                recs.append(T.tm_wire([b"t", b"X", b"m", b'{"a":"%s"}' % filler, b"{}"], j))
    got, data, off, _ = run(codec, recs)
    n = 128 * 16
    assert got["cm"].size == n  # no lead record: batch index == lane + 64 * tile
    raw, ends = data.tobytes(), set()
    for i in range(63, n, 128):  # lane 63 of an even tile: the key's value and '}' end the tile's window
        assert raw[int(off[i + 1]) - 9:int(off[i + 1])] == b':"alpha"}' and got["topic_idx"][i] == 1
        b = int(off[i + 1]) - 7 - int(off[i])
        assert (int(got["topic_off"][i]), int(got["topic_len"][i])) == (b, 5)
        ends.add(int(off[i + 1]) % 16)
    for i in range(64, n, 128):  # lane 0 of the next tile: the key starts 34 bytes into its window
        assert raw[int(off[i]) + 34:int(off[i]) + 41] == b'"topic"' and got["topic_idx"][i] == 2
    assert len(ends) >= 8  # the window's end sweeps the chunk phases
    idx = got["topic_idx"].reshape(16, 128)
    assert (idx[:, 63] == 1).all() and (idx[:, 64] == 2).all()
    assert int((got["topic_src"] == A.FALLBACK).sum()) == n - 32


def test_tiles_of_several_windows(codec):
    """Tiles whose 64 records exceed one LDS window: every record carries the key, so the ones
    around each window boundary do too; plus records just under and over the window size."""
    recs = []
    for i in range(64 * 3 + 5):
        fill = b"y" * (180 + 37 * (i % 7))
        recs.append(T.tm_wire([b"t", b"X", b"m%d" % i, b'{"f":"%s","topic":"beta"}' % fill,
                               b'{"pad":"%s","topic":"alpha"}' % fill if i % 2 else b"{}"], i))
    # records of size + 64 bytes: 16368 is the longest one that is staged, 16369 the first read from HBM
    for size in (16000, 16303, 16304, 16305, 16320, 17000):
        big = T.tm_wire([b"t", b"X", b"big", b'{"f":"%s","topic":"beta"}' % (b"z" * size), b"{}"], size)
        assert len(big) == size + 64
        recs.insert(70, big)
    got, _, _, _ = run(codec, recs, lead=7)
    assert (got["cm"][1:] == A.COMMIT).all() and set(got["topic_idx"][1:]) == {1, 2}


def test_long_records(codec):
    """Records longer than the window (the HBM reader) among short ones of the same tile."""
    short = [T.tm_wire([b"t", b"X", b"m%d" % i, A.P, b'{"topic":"alpha"}' if i % 5 == 0 else b"{}"], i)
             for i in range(40)]
    long_pl = T.tm_wire([b"t", b"X", b"L1", b'{"f":"%s","topic":"beta"}' % (b"p" * 19970), b"{}"], 1)
    long_hd = T.tm_wire([b"t", b"X", b"L2", A.P, b'{"f":"%s","topic":"alpha"}' % (b"h" * 19970)], 2)
    long_no = T.tm_wire([b"t", b"X", b"L3", b'{"f":"%s"}' % (b"n" * 19970), b"{}"], 3)
    long_esc = T.tm_wire([b"t", b"X", b"L4", b'{"f":"%s","t\\u006fpic":"_ack"}' % (b"e" * 19970), b"{}"], 4)
    recs = short[:10] + [long_pl] + short[10:20] + [long_hd, long_no] + short[20:30] + [long_esc] + short[30:]
    got, _, _, _ = run(codec, recs, lead=3)
    # (after the lead record) the long payload, the long headers, the long one without a key, the escaped key
    assert list(got["topic_idx"][[11, 22, 23]]) == [2, 1, 0] and got["cm"][34] == A.SKIP_TOPIC


def test_mixed_record_kinds(codec):
    tm = T.tm_wire([b"t", b"X", b"m1", A.P, b'{"topic":"alpha"}'], 5)
    recs = []
    for i in range(70):
        recs += [T.ack_wire(b"id%d" % i, b"orders", b"c", 5), T.session_event(i, 9, 7, 1, 0, b'{"topic":"alpha"}'),
                 T.session_wrap(tm), b"", b"\x01", T.hdr_bytes(16, 77, 1, 1) + b"\0" * 16, tm[:-3], T.simple_ack(9)]
    got, _, _, dec = run(codec, recs)
    assert (dec["flags"][6::8] & 0x4).all()  # SBE_FL_HEADERS_E100: headers = "", the fallback topic
    assert list(got["cm"][:8]) == [A.SKIP_TYPE, A.NO_ID, A.COMMIT, A.NOT_PARSED, A.NOT_PARSED, A.NOT_PARSED,
                                   A.COMMIT, A.SKIP_TYPE]
    assert got["topic_idx"][2] == 1 and got["topic_idx"][6] == 0


def test_tables(codec):
    names = [b"t%02d" % j for j in range(64)]
    vals = names + [b"absent", b"t\\u0030\\u0035", b"17", b"t63", b"t00"]
    recs = [T.tm_wire([b"t", b"X", b"m%d" % i, A.P, b'{"topic":"%s"}' % v if v != b"17" else b'{"topic":17}'], i)
            for i, v in enumerate(vals)]
    recs.append(T.tm_wire([b"t", b"X", b"mf", A.P, b"{}"], 99))
    got, _, _, _ = run(codec, recs, topics=names)
    assert list(got["topic_idx"]) == list(range(64)) + [A.UNKNOWN, 5, A.HOST, 63, 0, 0]
    assert got["count"][64] == 1 and got["count"][65] == 1 and got["last"][0] == 69 and got["last"][63] == 67
    # K = 1: only the fallback entry; a topic naming it resolves to 0 too
    got1, _, _, _ = run(codec, recs, topics=[b"t07"])
    assert got1["topic_idx"][7] == 0 and got1["topic_idx"][8] == A.UNKNOWN and got1["last"][0] == 69
    # duplicates: the first entry wins; a fallback topic that is _control
    got2, _, _, _ = run(codec, recs, topics=[b"_control", b"t01", b"t01", b"t00"])
    assert got2["topic_idx"][1] == 1 and got2["count"][2] == 0 and got2["cm"][69] == A.SKIP_CONTROL
    assert got2["last"][2] == U64MAX


def test_last_and_count_and_repeat(codec):
    r = A.random_records(64 * 3 + 5, 41)
    data, off = T.pack_records(r)
    exp_dec = T.oracle_decode(data, off, T.DEC_PARSE)
    exp = A.ref_classify(data, off, exp_dec, A.TOPICS)
    d, ro = to_dev(data, torch.uint8), to_dev(np.asarray(off, np.uint64), torch.int64)
    dec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE)
    plan = codec.classify_commits(d, ro, dec, A.TOPICS)
    torch.cuda.synchronize()
    first = plan.numpy()
    again = codec.classify_commits(d, ro, dec, A.TOPICS, out=plan)  # the same buffers
    torch.cuda.synchronize()
    assert_same(first, exp, data, off)
    assert_same(again.numpy(), exp, data, off)
    assert int(first["count"].sum()) == int((first["cm"] == A.COMMIT).sum()) > 20


def test_empty_batch(codec):
    got, exp, _ = classify(codec, np.zeros(0, np.uint8), np.zeros(1, np.uint64), A.TOPICS)
    assert_same(got, exp)
    assert (got["last"] == U64MAX).all() and (got["count"] == 0).all() and got["cm"].size == 0


def test_fixed256_orders(codec):
    n = 20000
    arena, L, ts = T.fixed256_orders(n)
    data, off, _ = T.oracle_encode(arena, L, ts)
    got, exp, _ = classify(codec, data, off, [b"orders", b"other"])
    assert_same(got, exp)
    assert (got["cm"] == A.COMMIT).all() and (got["topic_src"] == A.FALLBACK).all() and (got["topic_idx"] == 0).all()
    assert got["last"][0] == n - 1 and got["count"][0] == n and got["count"][1:].sum() == 0


def test_einval_writes_nothing(codec):
    recs = A.hand_records()[:40]
    data, off = T.pack_records(recs)
    d, ro = to_dev(data, torch.uint8), to_dev(np.asarray(off, np.uint64), torch.int64)
    dec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE)
    arena, toff = codec.commit_topic_table(A.TOPICS, d.device)
    n, k = len(recs), len(A.TOPICS)
    # every output with a sentinel; the u32 / u64 arrays over-allocated so they can be misaligned
    bufs = {f: torch.full(((n + 70) * {"uint8": 1, "uint32": 4, "uint64": 8}[t] + 8,), 0xA5, dtype=torch.uint8, device=d.device)
            for f, t in codec._COMMIT_KEYS}
    roff = torch.zeros(8 * (n + 1) + 8, dtype=torch.uint8, device=d.device)
    roff[4: 4 + 8 * (n + 1)] = ro.view(torch.uint8)
    toff_mis = torch.zeros(4 * (k + 1) + 4, dtype=torch.uint8, device=d.device)
    vo_mis = torch.zeros(dec.view_off.numel() * 4 + 4, dtype=torch.uint8, device=d.device)
    torch.cuda.synchronize()

    def call(**kw):
        a = dict(data=d.data_ptr(), rec_off=ro.data_ptr(), status=dec.status.data_ptr(), flags=dec.flags.data_ptr(),
                 view_off=dec.view_off.data_ptr(), view_len=dec.view_len.data_ptr(), arena=arena.data_ptr(),
                 toff=toff.data_ptr(), k=k, dec=True, out=True, **{f: b.data_ptr() for f, b in bufs.items()})
        a.update(kw)
        dd = codec._Decoded(a["status"], a["flags"], dec.hdr.data_ptr(), dec.ts.data_ptr(), a["view_off"],
                            a["view_len"], None)
        oo = codec._CommitOut(*(a[f] for f, _ in codec._COMMIT_KEYS))
        rc = codec.lib().sbe_classify_commits(a["data"], a["rec_off"], n, ctypes.byref(dd) if a["dec"] else None,
                                              a["arena"], a["toff"], a["k"], ctypes.byref(oo) if a["out"] else None,
                                              None, 0, None)
        torch.cuda.synchronize()
        return rc

    cases = [dict(data=None), dict(rec_off=None), dict(dec=False), dict(status=None), dict(flags=None),
             dict(view_off=None), dict(view_len=None), dict(arena=None), dict(toff=None), dict(out=False),
             dict(k=0), dict(k=65), dict(rec_off=roff.data_ptr() + 4), dict(toff=toff_mis.data_ptr() + 2),
             dict(view_off=vo_mis.data_ptr() + 1), dict(view_len=vo_mis.data_ptr() + 2)]
    cases += [{f: None} for f, _ in codec._COMMIT_KEYS]
    cases += [{f: bufs[f].data_ptr() + 2} for f in ("topic_off", "topic_len", "topic_idx")]
    cases += [{f: bufs[f].data_ptr() + 4} for f in ("last", "count")]
    for c in cases:
        assert call(**c) == -1, c  # SBE_EINVAL
    for f, b in bufs.items():
        assert bool((b == 0xA5).all()), f
    assert call() == 0
    assert not bool((bufs["cm"][:n] == 0xA5).all())


def test_autocommitter_host_program(codec):
    d = os.path.join(HERE, "autocommit")
    subprocess.run(["make", "-s", "-C", d, "test_autocommit_host"], check=True)
    r = subprocess.run([os.path.join(d, "test_autocommit_host")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "autocommit host test: ok" in r.stdout
