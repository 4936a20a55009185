"""GPU: the device kernels against the reference's own compiled flyweights (oracle/_ref, built by
build() where the reference tree is present), live and with no oracle in between: seeded random
encodes, mutated records through the three flyweight decode sequences, the Lite templates, and the
reference as the reader of what publish_orders_batch and emit_commit_offsets write.  The
generators are those of tests/test_oracle_vs_ref.py and tests/test_oracle_lite.py under seeds those
files do not use; here all records of a test go to the device as one batch, so a mutated record
sits inside a tile among valid ones.  Every comparison is exact.

Each differential asserts that its input cannot hide a failure: few records left out by the
precondition, a fair share of successes and of failures in the reference, enough headers-E100
records."""
import functools
import struct

import numpy as np
import pytest
import torch

import commitsend_lib as C
import golden_lib as G
import publish_lib as P
import sbe_testlib as T
from test_gpu_commit_emit import Dev
from test_gpu_frames import lite_gpu
from test_gpu_parity import SHAPES, gpu_decode, gpu_encode
from test_oracle_lite import mutate_lite, rand_lite_inputs
from test_oracle_vs_ref import mutate, rand_fields

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not T.ref_available(), reason="oracle/_ref not built (needs the reference tree)")]


def fair_mix(n_generated, ok):
    """ok: the reference's verdict on every kept record.  At most 5 % left out, at least a quarter
    of the kept records succeed and at least a quarter fail."""
    kept, good = len(ok), sum(1 for x in ok if x)
    assert kept >= 0.95 * n_generated, (kept, n_generated)
    assert good >= 0.25 * kept and kept - good >= 0.25 * kept, (good, kept)


# ------------------------------------------------------------------------------------------
# encode
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def encode_inputs():
    """2000 rand_fields records; about one in 50 has one field of 65534 / 65535 / 65536 / 70000
    bytes (the last valid length, E109, and the lengths publish_topic wraps)."""
    rng = np.random.default_rng(0x6E01)
    recs = [rand_fields(rng) for _ in range(2000)]
    long_at = {}
    for i in np.nonzero(rng.random(2000) < 0.02)[0]:
        k, ln = int(rng.integers(0, 5)), int(rng.choice([65534, 65535, 65536, 70000]))
        recs[i][k] = bytes(rng.integers(0, 256, ln, dtype=np.uint8))
        long_at[int(i)] = (k, ln)
    ts = rng.integers(1, 2**64 - 1, len(recs), dtype=np.uint64)
    L = np.array([[len(f) for f in r] for r in recs], np.uint32)
    arena = np.frombuffer(b"".join(b"".join(r) for r in recs), np.uint8)
    return recs, ts, L, arena, long_at


def device_records(codec, flags):
    recs, ts, L, arena, _ = encode_inputs()
    out, off, st = gpu_encode(codec, arena, L, ts, flags=flags)
    out = out.tobytes()
    return [out[int(off[i]):int(off[i + 1])] for i in range(len(recs))], st


@pytest.mark.parametrize("flags,wire", [(0, True), (T.ENC_REF_TRUNCATE8, False)])
def test_encode_random_vs_ref(codec, flags, wire):
    recs, ts, _, _, long_at = encode_inputs()
    got, st = device_records(codec, flags)
    n_e109 = 0
    for i, r in enumerate(recs):
        rc, ref = T.ref_encode(r, int(ts[i]), wire=wire)
        assert int(st[i]) == rc and got[i] == ref, (i, int(st[i]), rc, len(got[i]), len(ref))
        n_e109 += rc != 0
    # the long fields are there: E109 on every length past 65534, the 65534-byte field encodes
    assert n_e109 == sum(1 for _, ln in long_at.values() if ln > 65534) >= 10
    assert sum(1 for _, ln in long_at.values() if ln == 65534) >= 3


def test_publish_random_vs_ref(codec):
    recs, ts, _, _, long_at = encode_inputs()
    got, st = device_records(codec, T.ENC_PUBLISH_TOPIC)
    for i, r in enumerate(recs):
        rc, ref = T.ref_publish(r, int(ts[i]))
        assert rc == 0 and int(st[i]) == 0 and got[i] == ref, (i, int(st[i]), len(got[i]), len(ref))
    assert sum(1 for _, ln in long_at.values() if ln >= 65536) >= 5  # lengths that wrap


# ------------------------------------------------------------------------------------------
# TopicMessage decode (parse and on_egress) and Acknowledgment decode
# ------------------------------------------------------------------------------------------
N_MUTATED = 3000


@functools.lru_cache(maxsize=None)
def tm_records():
    """(all generated records, indices kept by the precondition, the reference's results for them)."""
    rng = np.random.default_rng(0x6E02)
    recs = [mutate(rng, T.tm_wire(rand_fields(rng), int(rng.integers(0, 2**63)))) for _ in range(N_MUTATED)]
    kept = [i for i, r in enumerate(recs) if len(r) >= 8 and r[2:6] == b"\x01\x00\x01\x00"]
    return recs, kept, [T.ref_tm_decode(recs[i]) for i in kept], [T.ref_egress_tm(recs[i]) for i in kept]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_tm_parse_mutated_vs_ref(codec, shape):
    recs, kept, parsed, _ = tm_records()
    fair_mix(N_MUTATED, [rc == 0 for rc, *_ in parsed])
    assert sum(1 for rc, _, _, hok in parsed if rc == 0 and not hok) >= 50
    d = gpu_decode(codec, *T.pack_records(recs), T.DEC_PARSE, in_bytes=SHAPES[shape])
    for i, (rc, ts, f, hok) in zip(kept, parsed):
        rec = recs[i]
        pr = T.materialize_parse(rec, T.row(d, i))
        assert pr["success"] == (rc == 0), (i, rec.hex())
        if rc == 0:
            assert pr["timestamp"] == T._i64(ts), i
            assert [pr["message_type"], pr["message_id"], pr["payload"]] == f[1:4], (i, rec.hex())
            assert pr["headers"] == (f[4] if hok else b""), (i, rec.hex())
            assert bool(int(d["flags"][i]) & T.FL_HEADERS_E100) == (not hok), (i, rec.hex())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_tm_egress_mutated_vs_ref(codec, shape):
    recs, kept, _, egress = tm_records()
    fair_mix(N_MUTATED, [rc == 0 for rc, _ in egress])
    d = gpu_decode(codec, *T.pack_records(recs), T.DEC_EGRESS, in_bytes=SHAPES[shape])
    for i, (rc, f) in zip(kept, egress):
        out = T.materialize_egress(recs[i], T.row(d, i))
        if rc:
            assert out == ("throw", b"buffer too short [E100]"), (i, recs[i].hex())
        elif f[0] == b"":
            assert out == ("none",), (i, recs[i].hex())
        else:
            assert out == ("tm", tuple(f)), (i, recs[i].hex())


@functools.lru_cache(maxsize=None)
def ack_records():
    rng = np.random.default_rng(0x6E03)
    recs = []
    for _ in range(N_MUTATED):
        f = rand_fields(rng)[:3]
        recs.append(mutate(rng, T.ack_wire(*f, int(rng.integers(0, 2**63))) + b"\0" * int(rng.integers(0, 12))))
    kept = [i for i, r in enumerate(recs) if not (len(r) < 16 or r[2:6] != b"\x02\x00\x01\x00" or
                                                  (len(r) == 16 and r[:2] == b"\x08\x00"))]
    return recs, kept, [T.ref_ack_decode(recs[i]) for i in kept]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_ack_mutated_vs_ref(codec, shape):
    recs, kept, acks = ack_records()
    fair_mix(N_MUTATED, [rc == 0 for rc, *_ in acks])
    d = gpu_decode(codec, *T.pack_records(recs), T.DEC_EGRESS, in_bytes=SHAPES[shape])
    for i, (rc, ts, fl) in zip(kept, acks):
        out = T.materialize_egress(recs[i], T.row(d, i))
        if rc:
            assert out[0] != "ack", (i, recs[i].hex())
        else:
            assert out[0] == "ack" and not out[1]["simple_control_ack"], (i, recs[i].hex())
            assert [out[1]["message_id"], out[1]["topic"], out[1]["correlation_id"]] == fl, (i, recs[i].hex())
            assert out[1]["timestamp_nanos"] == G.to_nanos_auto(ts), i


# ------------------------------------------------------------------------------------------
# Lite templates
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [301, 201, 202])
def test_lite_random_vs_ref(codec, t):
    """300 random records per template (900 in all): the device's encode against ref_lite_encode,
    then mutations of the reference's records through DEC_LITE against ref_lite_decode."""
    rng = np.random.default_rng(0x6E00 + t)
    nf, n = T.LITE_NF[t], 300
    fields, tid, seq = rand_lite_inputs(rng, t, n)
    L = np.array([[len(f) for f in r] for r in fields], np.uint32)
    arena = np.frombuffer(b"".join(b"".join(r) for r in fields), np.uint8)
    out, off, st = lite_gpu(codec, t, arena, L, tid, seq)
    out = out.tobytes()
    recs = []
    for i in range(n):
        rc, ref = T.ref_lite_encode(t, fields[i], int(tid[i]), int(seq[i]))
        assert rc == 0 and int(st[i]) == 0 and out[int(off[i]):int(off[i + 1])] == ref, i
        recs.append(mutate_lite(rng, ref))
    refs = [T.ref_lite_decode(r) for r in recs]
    fair_mix(n, [rc == 0 for rc, *_ in refs])
    d = gpu_decode(codec, *T.pack_records(recs), T.DEC_LITE)
    for i, (r, (rc, rtid, rseq, f)) in enumerate(zip(recs, refs)):
        row = T.row(d, i)
        if rc:
            assert row["status"] == T.ST_LITE_E100, (i, r.hex())
            continue
        assert row["status"] == T.ST_LITE and int(row["ts"]) == rseq and int(row["view_off"][4]) == rtid, (i, r.hex())
        for k in range(nf):
            o, m = int(row["view_off"][k]), int(row["view_len"][k])
            assert r[o:o + m] == f[k], (i, k, r.hex())


# ------------------------------------------------------------------------------------------
# the reference reads what the device writes downstream
# ------------------------------------------------------------------------------------------
def session_header(term, sess):
    """include/sbecodec.h: {24, 1, 111, 8}, i64 leadershipTermId, i64 clusterSessionId, i64 0."""
    return struct.pack("<4Hqqq", 24, 1, 111, 8, term, sess, 0)


@pytest.mark.parametrize("flags", [0, T.ENC_REF_TRUNCATE8])
@pytest.mark.parametrize("session", [False, True])
def test_published_orders_read_by_ref(codec, session, flags):
    """publish_orders_batch's records parsed by the reference's TopicMessage flyweight: topic,
    message type, uuid and timestamp as given, payload and headers the texts order_to_json_batch
    returns for the same Orders.  This pins the framing; the JSON text itself stays unpinned
    (jsoncpp absent).  Under ENC_REF_TRUNCATE8 (the live path) the reference loses the headers to
    E100, as it does for its own encoder's records."""
    n, topic, term, sess, ts_default = 257, b"orders", -5, 2**40 + 9, 424242
    b = P.mixed_batch(n, 0x6E04)
    tm_ts = np.arange(n, dtype=np.uint64) % 3 * 1_000_003  # every third record takes ts_default
    out, off, st, _ = P.run_device(codec, b, topic, tm_ts, ts_default, flags, session, term=term, sess=sess)
    arena, str_len = T.pack_order_fields(b.fields)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    texts = []
    for what in (codec.JSON_ORDER_PAYLOAD, codec.JSON_PUBLISH_HEADERS):
        j = codec.order_to_json_batch(dev(arena, np.uint8), dev(str_len, np.int32), dev(b.cid, np.int64),
                                      dev(b.ts, np.int64), dev(b.q, np.float64), what=what)
        torch.cuda.synchronize()
        jo, text = j.out_off.cpu().numpy(), j.out.cpu().numpy().tobytes()
        assert (j.status.cpu().numpy()[:n] == codec.JSON_OK).all()
        texts.append([text[int(jo[i]):int(jo[i + 1])] for i in range(n)])
    out, hdr, read = out.tobytes(), session_header(term, sess) if session else b"", 0
    for i in range(n):
        rec = out[int(off[i]):int(off[i + 1])]
        if st[i] != 0:
            assert st[i] >= P.INVALID_BASE and rec == b"", (i, st[i])  # refused by validate(): no bytes
            continue
        assert rec[: len(hdr)] == hdr, i
        rc, ts, f, hok = T.ref_tm_decode(rec[len(hdr):])
        assert rc == 0, i
        upd = b.fields[i][P.F_STATUS] in (b"UPDATED", b"CANCELLED")
        assert f[:4] == [topic, b"UPDATE_ORDER" if upd else b"CREATE_ORDER", b.fields[i][P.F_MSGID], texts[0][i]], i
        assert ts == (int(tm_ts[i]) or ts_default), i
        if flags:
            assert not hok, i
        else:
            assert hok and f[4] == texts[1][i], i
        read += 1
    assert read == int((b.masks() == 0).sum()) >= n // 16  # every order validate() passes was read back


def named_frames(b):
    """What commitsend_lib / autocommit_lib name for every record with a frame: (record, topic id,
    sequence, message id, identifier), the selection of commitsend_lib.ref_emit."""
    exp = b.expected()
    for i in (int(x) for x in exp["emit_idx"]):
        j = int(b.plan["topic_idx"][i])
        o, ln = int(b.off[i]) + int(b.dec["view_off"][i, 2]), int(b.dec["view_len"][i, 2])
        has = b.dec["status"][i] == T.ST_TM and b.dec["flags"][i] & (T.FL_SEQ_KEY | T.FL_SEQ_ESC)
        yield i, C.TOPIC_IDS[j], int(b.seq[i]) if has else 0, bytes(b.data[o:o + ln]), C.IDENTS[j]


@pytest.mark.parametrize("session", [False, True])
@pytest.mark.parametrize("which", ["hand", "random"])
def test_commit_frames_read_by_ref(codec, which, session):
    """emit_commit_offsets' frames parsed by the reference's CommitOffsetLite flyweight."""
    term, sess = 3, -4
    b = Dev(codec, C.hand_records() if which == "hand" else C.random_records())
    got = b.run(session=session, term=term, sess=sess)
    named = list(named_frames(b))
    assert [i for i, *_ in named] == [int(x) for x in got["emit_idx"]]
    assert len(named) >= (8 if which == "hand" else 500)
    out, hdr = got["out"].tobytes(), session_header(term, sess) if session else b""
    for i, tid, seq, mid, ident in named:
        frame = out[int(got["out_off"][i]):int(got["out_off"][i + 1])]
        assert got["status"][i] == C.EMITTED and frame[: len(hdr)] == hdr, i
        lite = frame[len(hdr):]
        assert struct.unpack("<4H", lite[:8]) == (12, 301, 1, 1), i
        rc, rtid, rseq, f = T.ref_lite_decode(lite)
        assert rc == 0 and (rtid, rseq, f[0], f[1]) == (tid, seq, mid, ident), (i, rtid, rseq, f[:2])
        if which == "hand":  # the message id as the hand table spells it
            assert mid == C.HAND[i][0][1], i
    if which == "hand":
        assert {s for _, _, s, _, _ in named} == {0, 123456789012}
