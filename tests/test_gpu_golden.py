"""GPU: every case of the golden fixtures (tests/golden/*.json, what the reference's own compiled
flyweights produced) through the device kernels, with the expectations of golden_lib, the same
functions the CPU tests run with the oracle as subject.  Expected values come from the fixture
files only: no oracle call stands in an assertion here, and neither the reference tree nor
oracle/_ref is needed.  Each test asserts that it reached every case of its file."""
import struct

import numpy as np
import pytest
import torch

import golden_lib as G
import sbe_testlib as T
from test_gpu_parity import SHAPES, gpu_decode, to_dev

pytestmark = pytest.mark.gpu

TERM, SESS = 0x0102030405060708, -7
# include/sbecodec.h: {blockLength 24, templateId 1, schemaId 111, version 8}, i64 leadershipTermId,
# i64 clusterSessionId, i64 timestamp 0
SESSION_HDR = struct.pack("<4Hqqq", 24, 1, 111, 8, TERM, SESS, 0)
ENCODE, PUBLISH = G.load("encode_ref.json")["cases"], G.load("publish_ref.json")["cases"]
TM, ACK, EGRESS = (G.load(f)["cases"] for f in ("decode_tm_ref.json", "ack_ref.json", "egress_tm_ref.json"))
LITE = G.load("lite_ref.json")
PROBES = G.load("survey_probes.json")["probes"]


@pytest.fixture(scope="module")
def server(codec):
    s = codec.Server()
    yield s
    s.close()


# ------------------------------------------------------------------------------------------
# input builders and the device subjects
# ------------------------------------------------------------------------------------------
def packed(fields_list, nf=5):
    L = np.array([[len(f) for f in r] for r in fields_list], np.uint32).reshape(-1, nf)
    return np.frombuffer(b"".join(b"".join(r) for r in fields_list), np.uint8), L, None


def gathered(fields_list, nf=5):
    """str_off input: every distinct string once, last record's first, behind ragged gaps."""
    at, where, pieces = 3, {}, [b"\xee" * 3]
    for r in reversed(fields_list):
        for f in r:
            if f not in where:
                where[f] = at
                gap = len(where) % 3
                pieces += [f, b"\xee" * gap]
                at += len(f) + gap
    L = np.array([[len(f) for f in r] for r in fields_list], np.uint32).reshape(-1, nf)
    off = np.array([[where[f] for f in r] for r in fields_list], np.uint32).reshape(-1, nf)
    return np.frombuffer(b"".join(pieces), np.uint8), L, off


def split(enc, n):
    """(records, out_off, statuses) of an Encoded; record i = out[out_off[i]:out_off[i+1]]."""
    off = enc.out_off.cpu().numpy().view(np.uint64)
    assert int(off[0]) == 0 and (np.diff(off.astype(np.int64)) >= 0).all()
    out = enc.out[: int(off[n])].cpu().numpy().tobytes()
    return [out[int(off[i]):int(off[i + 1])] for i in range(n)], off, [int(s) for s in enc.status.cpu().numpy()[:n]]


class DevEncode:
    """encode(fields_list, ts_list, flags) on the device, all records in one batch.  how: "packed" /
    "gather" (encode_topic_batch), "session" (encode_session_batch; the 32 header bytes are checked
    and taken off), "serve" (Server.encode_topic).  offs keeps (flags, out_off) of every call."""

    def __init__(self, codec, how, server=None):
        self.codec, self.how, self.server, self.offs = codec, how, server, []

    def __call__(self, fields_list, ts_list, flags):
        n = len(ts_list)
        arena, L, off = (gathered if self.how == "gather" else packed)(fields_list)
        a = to_dev(arena if arena.size else np.zeros(16, np.uint8), torch.uint8)
        Ld, t = to_dev(L, torch.int32), to_dev(np.array(ts_list, np.uint64), torch.int64)
        if self.how == "session":
            enc = self.codec.encode_session_batch(a, Ld, t, TERM, SESS, flags=flags)
        elif self.how == "serve":
            enc = self.server.encode_topic(a, Ld, t, flags=flags)
        elif off is None:
            enc = self.codec.encode_topic_batch(a, Ld, t, flags=flags)
        else:  # strings shared between records: the output is sized from the lengths, not from the arena
            out = torch.empty(self.codec.output_bound(n, int(L.sum(dtype=np.uint64)), flags) + 16, dtype=torch.uint8,
                              device="cuda")
            enc = self.codec.encode_topic_batch(a, Ld, t, str_off=to_dev(off, torch.int32), flags=flags, out=out)
        torch.cuda.synchronize()
        recs, out_off, st = split(enc, n)
        self.offs.append((flags, out_off))
        if self.how == "session":
            for i, r in enumerate(recs):
                assert r[:32] == SESSION_HDR[: len(r)], (i, r[:32].hex())  # b"" for a record without output
            recs = [r[32:] for r in recs]
        return recs, st


def expected_off(cases, key, status=lambda c: c["status"], extra=0):
    """out_off from the fixture alone: cumulative record lengths, 0 bytes for an E109 case."""
    off = np.zeros(len(cases) + 1, np.uint64)
    off[1:] = np.cumsum([G.blob_len(c[key]) + extra if status(c) == 0 else 0 for c in cases])
    return off


def check_offs(enc, cases, key_of_flags, **kw):
    assert enc.offs, "the subject was never called"
    for flags, off in enc.offs:
        np.testing.assert_array_equal(off, expected_off(cases, key_of_flags[flags], **kw))


def tile_positions(idx, n, tile):
    """How many distinct places of a `tile`-record tile each of the n cases takes in the batch idx."""
    pos = [set() for _ in range(n)]
    for j, c in enumerate(idx):
        pos[c].add(j % tile)
    return [len(p) for p in pos]


def rotated(cases, tile):
    """The case list repeated, repetition r rotated by 5 r, until the batch spans three tiles of
    `tile` records and every case has stood at three or more places of a tile."""
    n, reps = len(cases), -(-3 * tile // len(cases))
    while True:
        idx = [(c + 5 * r) % n for r in range(reps) for c in range(n)]
        if min(tile_positions(idx, n, tile)) >= 3:
            break
        reps += 1
    assert len(idx) >= 3 * tile and len(idx) % n == 0 and min(tile_positions(idx, n, tile)) >= 3
    assert sorted(idx) == sorted(list(range(n)) * reps)  # every case, the same number of times
    return [cases[c] for c in idx]


def largest_tile(codec):
    return max(int(codec.lib().sbe_encode_tile_records(l))
               for l in (codec.LAYOUT_TOPIC, codec.LAYOUT_SESSION, codec.LAYOUT_LITE))


ENCODE_KEYS = {0: "wire", T.ENC_REF_TRUNCATE8: "ref_truncated"}
PUBLISH_KEYS = {T.ENC_PUBLISH_TOPIC: "record"}
NO_E109 = dict(status=lambda c: 0)


# ------------------------------------------------------------------------------------------
# encode_ref.json (22 cases) and publish_ref.json (28 cases)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["packed", "gather", "session", "serve"])
def test_encode_ref_cases(codec, server, how):
    """All cases as one batch under flags 0 and ENC_REF_TRUNCATE8: status, out_off and every byte."""
    assert len(ENCODE) == 22
    enc = DevEncode(codec, how, server)
    assert G.check_encode_ref(ENCODE, enc) == 22
    assert sorted(f for f, _ in enc.offs) == [0, T.ENC_REF_TRUNCATE8]
    check_offs(enc, ENCODE, ENCODE_KEYS, extra=32 if how == "session" else 0)


@pytest.mark.parametrize("how", ["packed", "gather", "session"])
def test_encode_ref_cases_at_every_tile_position(codec, how):
    """The case list repeated under a rotation: three tiles and more, every case at three or more
    places of a tile, so a case's bytes must not depend on where in a tile it stands or on what
    stands before it (the E109 cases put nothing out; the 65534-byte case spans windows)."""
    cases = rotated(ENCODE, largest_tile(codec))
    assert len(cases) % 22 == 0 and len(cases) >= 3 * largest_tile(codec)
    enc = DevEncode(codec, how)
    assert G.check_encode_ref(cases, enc) == len(cases)
    check_offs(enc, cases, ENCODE_KEYS, extra=32 if how == "session" else 0)


@pytest.mark.parametrize("how", ["packed", "gather", "serve"])
def test_publish_ref_cases(codec, server, how):
    """ENC_PUBLISH_TOPIC against `record` (encode_session_batch refuses the flag: publish_topic
    does not go through the session framing)."""
    assert len(PUBLISH) == 28
    enc = DevEncode(codec, how, server)
    assert G.check_publish_ref(PUBLISH, enc) == 28
    check_offs(enc, PUBLISH, PUBLISH_KEYS, **NO_E109)


@pytest.mark.parametrize("how", ["packed", "gather"])
def test_publish_ref_cases_at_every_tile_position(codec, how):
    cases = rotated(PUBLISH, largest_tile(codec))
    assert len(cases) % 28 == 0 and len(cases) >= 3 * largest_tile(codec)
    enc = DevEncode(codec, how)
    assert G.check_publish_ref(cases, enc) == len(cases)
    check_offs(enc, cases, PUBLISH_KEYS, **NO_E109)


# ------------------------------------------------------------------------------------------
# decode_tm_ref.json / ack_ref.json / egress_tm_ref.json
# ------------------------------------------------------------------------------------------
def dev_decode(codec, shape, lead):
    """decode(records, mode): one batch under the window shape, behind `lead` bytes (a record of
    their own in front, as in test_gpu_parity's alignment tests; its row is dropped)."""
    def decode(recs, mode):
        data, off = T.pack_records([b"\0" * lead] + list(recs))
        d = gpu_decode(codec, data, off, mode, in_bytes=SHAPES[shape])
        return {k: v[1:] for k, v in d.items()}
    return decode


def serve_decode(server):
    def decode(recs, mode):
        data, off = T.pack_records(list(recs))
        d = to_dev(data if data.size else np.zeros(16, np.uint8), torch.uint8)
        return server.decode(d, to_dev(off, torch.int64), mode=mode).numpy()
    return decode


def decode_subjects(codec, shape):
    return [dev_decode(codec, shape, lead) for lead in range(16)]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_parse_tm_cases(codec, shape):
    for decode in decode_subjects(codec, shape):
        assert G.check_parse_tm(TM, decode) == len(TM)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_decode_ack_cases(codec, shape):
    for decode in decode_subjects(codec, shape):
        assert G.check_decode_ack(ACK, decode) == len(ACK)


def check_egress(decode):
    checked, claimed = G.check_egress_tm(EGRESS, decode, check_rec=True)
    # decode_ack may claim no more of these records than it does with the oracle as subject
    assert claimed <= G.EGRESS_TM_ACK_CLAIMED and checked + claimed == len(EGRESS)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_on_egress_tm_cases(codec, shape):
    for decode in decode_subjects(codec, shape):
        check_egress(decode)


def test_decode_cases_served(codec, server):
    decode = serve_decode(server)
    assert G.check_parse_tm(TM, decode) == len(TM)
    assert G.check_decode_ack(ACK, decode) == len(ACK)
    check_egress(decode)


def test_fixture_files_are_not_empty():
    """The counts the tests above compare with are the files' own; this pins them, and that each
    file holds both outcomes."""
    assert (len(ENCODE), len(PUBLISH), len(TM), len(ACK), len(EGRESS)) == (22, 28, 58, 51, 58)
    assert sum(1 for c in TM if not c["e100"]) == 18 and sum(1 for c in TM if c["headers_ok"] == 0) == 4
    assert sum(1 for c in ACK if not c["fails"]) == 6 and sum(1 for c in EGRESS if c["throws"]) == 51
    assert len(LITE["encode"]) == 20 and len(LITE["decode"]) == 96 and len(PROBES) == 16
    assert sum(1 for c in LITE["decode"] if c["e100"]) == 84


@pytest.mark.parametrize("shape", ["w16k", "w8k"])
def test_materialized_tm_cases(codec, shape):
    """materialize_views over the decode_tm_ref cases that succeed: the strings in the device arena
    against the fixture's fields."""
    def views(recs):
        data, off = T.pack_records(list(recs))
        d, r = to_dev(data, torch.uint8), to_dev(off, torch.int64)
        dec = codec.decode_batch(d, r, mode=codec.DEC_PARSE_MESSAGE, in_bytes=SHAPES[shape](len(recs)))
        m = codec.materialize_views(d, r, dec)
        torch.cuda.synchronize()
        assert (dec.status.cpu().numpy() == T.ST_TM).all()
        arena, ao = m.arena.cpu().numpy().tobytes(), m.arena_off.cpu().numpy().view(np.uint64)
        assert ao.size == 5 * len(recs) + 1 and int(ao[0]) == 0
        return [tuple(arena[int(ao[5 * i + k]):int(ao[5 * i + k + 1])] for k in range(5)) for i in range(len(recs))]

    n_ok = sum(1 for c in TM if not c["e100"])
    assert G.check_materialized_tm(TM, views) == n_ok


# ------------------------------------------------------------------------------------------
# lite_ref.json
# ------------------------------------------------------------------------------------------
def dev_lite_encode(codec, how, server=None):
    def lite_encode(t, fields_list, tids, seqs):
        nf = T.LITE_NF[t]
        arena, L, off = (gathered if how == "gather" else packed)(fields_list, nf)
        a = to_dev(arena if arena.size else np.zeros(16, np.uint8), torch.uint8)
        args = (t, a, to_dev(L, torch.int32), to_dev(np.array(tids, np.uint32), torch.int32),
                to_dev(np.array(seqs, np.uint64), torch.int64))
        if how == "serve":
            enc = server.encode_lite(*args)
        elif off is None:
            enc = codec.encode_lite_batch(*args)
        else:
            cap = int(codec.lib().sbe_lite_output_bound(len(seqs), int(L.sum(dtype=np.uint64)), t))
            enc = codec.encode_lite_batch(*args, str_off=to_dev(off, torch.int32),
                                          out=torch.empty(cap + 16, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        recs, _, st = split(enc, len(seqs))
        return recs, st
    return lite_encode


@pytest.mark.parametrize("how", ["packed", "gather", "serve"])
def test_lite_encode_cases(codec, server, how):
    assert G.check_lite_encode(LITE["encode"], dev_lite_encode(codec, how, server)) == 20


@pytest.mark.parametrize("shape", list(SHAPES))
def test_lite_decode_cases(codec, shape):
    for decode in decode_subjects(codec, shape):
        assert G.check_lite_decode(LITE["decode"], decode) == 96


def test_lite_decode_cases_served(codec, server):
    assert G.check_lite_decode(LITE["decode"], serve_decode(server)) == 96


# ------------------------------------------------------------------------------------------
# survey_probes.json
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["batch", "serve"])
def test_survey_probes(codec, server, how):
    if how == "batch":
        encode, decode = DevEncode(codec, "packed"), dev_decode(codec, "w16k", 0)
    else:
        encode, decode = DevEncode(codec, "serve", server), serve_decode(server)
    assert G.check_survey_probes(PROBES, encode, decode) == 16


# ------------------------------------------------------------------------------------------
# parse_ref.json
# ------------------------------------------------------------------------------------------
PARSE = G.parse_ref_cases()


@pytest.mark.parametrize("lead", [0, 1, 15])
def test_parse_ref_cases(codec, lead):
    """The device as subject: decode_batch with the fused sequence number and sbe_order_select over
    the fixture's records as one batch behind `lead` bytes."""
    def parse(recs):
        data, off = T.pack_records([b"\0" * lead] + list(recs))
        d, ro = to_dev(data, torch.uint8), to_dev(off, torch.int64)
        dec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE, seq=True)
        pred = codec.order_select(d, ro, dec).numpy()["pred"]
        torch.cuda.synchronize()
        return {k: v[1:] for k, v in dec.numpy().items()}, dec.seq.cpu().numpy().view(np.uint64)[1:], pred[1:]
    assert G.check_parse_ref(PARSE, parse) == len(PARSE) >= 150


def test_parse_ref_cases_host_mirror(codec, tmp_path):
    """The host mirror as subject (tests/cpp/test_parse_lines.cpp, one parse_message call per
    record): its predicates and ParseResult::get_description against the fixture's."""
    import refsrc_lib as R
    lines = R.mirror_lines([bytes.fromhex(c["rec"]) for c in PARSE], "single", tmp_path)
    for c, ln in zip(PARSE, lines):
        kv = dict(x.split("=", 1) for x in ln.split(" "))
        assert bytes.fromhex(kv["desc"]) == c["desc"].encode("latin-1") and int(kv["pred"][::-1], 2) == c["pred"], (c["name"], kv["desc"], kv["pred"])
        assert kv["ok"] == str(c["result"][0]), c["name"]
