"""The expectations of the golden fixtures (tests/golden/*.json: what the reference's own compiled
flyweights produced, and the SURVEY Appendix B probe observations), stated once for two subjects:
the oracle restatement (tests/test_oracle_golden.py, tests/test_oracle_lite.py; CPU) and the device
kernels (tests/test_gpu_golden.py).  A subject is a set of callables:

  encode(fields_list, ts_list, flags) -> (records [bytes], statuses [int])
  decode(records [bytes], mode)       -> descriptor arrays as T.oracle_decode returns them (record i
                                         is T.row(d, i), ready for T.materialize_parse / _egress)
  lite_encode(template, fields_list, topic_ids, sequences) -> (records [bytes], statuses [int])

Every check_* function takes a list of fixture cases and returns how many it checked, so a caller
can assert that nothing was filtered away.  Expected values come from the fixture files only; the
oracle_* functions at the end are the CPU subject."""
import hashlib
import json
import os
import struct

import numpy as np

import sbe_testlib as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F5 = [b"orders", b"CREATE_ORDER", b"msg_1", b'{"a":1}', b'{"h":2}']
PROBE_TS = 0x1122334455667788
# the encode_ref probes of survey_probes.json: name -> the five strings
ENCODE_PROBE_FIELDS = {"encode_appendix_b": F5, "encode_all_empty": [b""] * 5,
                       "encode_empty_headers": F5[:4] + [b""], "encode_topic_65535": [b"x" * 65535] + F5[1:]}
# egress_tm_ref.json cases that decode_ack claims before on_egress reaches the TopicMessage branch,
# with the oracle as subject: none (decode_ack wants template 2, src/ack_decoder.cpp:40-42, and the
# fixture holds template-1 records only).  tests/test_oracle_golden.py asserts the number.
EGRESS_TM_ACK_CLAIMED = 0


def load(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


def same(blob, b):
    b = bytes(b)
    if isinstance(blob, str):
        return bytes.fromhex(blob) == b
    return (blob["len"] == len(b) and blob["sha256"] == hashlib.sha256(b).hexdigest())


def blob_len(blob):
    return len(blob) // 2 if isinstance(blob, str) else blob["len"]


def fields_of(spec):
    return [bytes([f["fill"]]) * f["len"] if isinstance(f, dict) else bytes.fromhex(f) for f in spec]


def to_nanos_auto(ts):
    """decode_ack's to_nanos_auto (src/ack_decoder.cpp): values below 1e14 are milliseconds."""
    return (ts * 1_000_000 if ts < 100_000_000_000_000 else ts) & (2**64 - 1)


def records_by_name():
    return dict(T.edge_records())


# ------------------------------------------------------------------------------------------
# encode_ref.json / publish_ref.json
# ------------------------------------------------------------------------------------------
def check_encode_ref(cases, encode):
    """SBEEncoder::encode_topic_message's flyweight sequence: ref_truncated under ENC_REF_TRUNCATE8,
    wire under 0, E109 cases with their status and no bytes."""
    fl, ts = [fields_of(c["fields"]) for c in cases], [int(c["ts"]) for c in cases]
    got_t, st_t = encode(fl, ts, T.ENC_REF_TRUNCATE8)
    got_w, st_w = encode(fl, ts, 0)
    assert len(got_t) == len(got_w) == len(st_t) == len(st_w) == len(cases)
    for i, case in enumerate(cases):
        assert st_t[i] == case["status"] and st_w[i] == case["status"], (i, st_t[i], st_w[i], case["status"])
        if case["status"] == 0:
            assert same(case["ref_truncated"], got_t[i]), (i, case["ts"])
            assert same(case["wire"], got_w[i]), (i, case["ts"])
        else:
            assert got_t[i] == b"" and got_w[i] == b"", (i, case["ts"])
    return len(cases)


def check_publish_ref(cases, encode):
    """SBE_ENC_PUBLISH_TOPIC against ClusterClient::publish_topic's own flyweight sequence
    (src/cluster_client.cpp:1823-1858): lengths mod 65536, no E109."""
    fl, ts = [fields_of(c["fields"]) for c in cases], [int(c["ts"]) for c in cases]
    got, st = encode(fl, ts, T.ENC_PUBLISH_TOPIC)
    assert len(got) == len(st) == len(cases)
    for i, case in enumerate(cases):
        assert st[i] == 0 and same(case["record"], got[i]), (i, case["ts"], st[i])
    return len(cases)


# ------------------------------------------------------------------------------------------
# decode_tm_ref.json / ack_ref.json / egress_tm_ref.json
# ------------------------------------------------------------------------------------------
def fixture_records(cases, check_rec=True):
    """The cases' records by name from T.edge_records(), checked against the fixture's rec blob."""
    by_name = records_by_name()
    recs = [by_name[c["name"]] for c in cases]
    if check_rec:
        for c, rec in zip(cases, recs):
            assert same(c["rec"], rec), c["name"]
    return recs


def check_parse_tm(cases, decode):
    recs = fixture_records(cases)
    d = decode(recs, T.DEC_PARSE)
    for i, (case, rec) in enumerate(zip(cases, recs)):
        pr = T.materialize_parse(rec, T.row(d, i))
        if case["e100"]:
            assert not pr["success"] and \
                pr["error_message"] == b"SBE TopicMessage decoding failed: buffer too short [E100]", case["name"]
            continue
        assert pr["success"] and pr["timestamp"] == T._i64(int(case["ts"])), case["name"]
        f = case["fields"]
        assert same(f[1], pr["message_type"]) and same(f[2], pr["message_id"]) and same(f[3], pr["payload"]), \
            case["name"]
        if case["headers_ok"]:
            assert same(f[4], pr["headers"]), case["name"]
        else:
            assert pr["headers"] == b"" and int(d["flags"][i]) & T.FL_HEADERS_E100, case["name"]
    return len(cases)


def check_decode_ack(cases, decode, to_nanos=to_nanos_auto):
    recs = fixture_records(cases)
    d = decode(recs, T.DEC_EGRESS)
    for i, (case, rec) in enumerate(zip(cases, recs)):
        out = T.materialize_egress(rec, T.row(d, i))
        if case["fails"]:
            assert out[0] != "ack", case["name"]
            continue
        assert out[0] == "ack" and not out[1]["simple_control_ack"], case["name"]
        assert out[1]["timestamp_nanos"] == int(to_nanos(int(case["ts"]))), case["name"]
        for k, key in enumerate(("message_id", "topic", "correlation_id")):
            assert same(case["fields"][k], out[1][key]), (case["name"], key)
    return len(cases)


def check_egress_tm(cases, decode, check_rec=False):
    """→ (cases checked, cases decode_ack claimed first): a claimed case is checked in ack_ref, not
    here, and is not among the checked ones."""
    recs = fixture_records(cases, check_rec)
    d = decode(recs, T.DEC_EGRESS)
    checked = claimed = 0
    for i, (case, rec) in enumerate(zip(cases, recs)):
        out = T.materialize_egress(rec, T.row(d, i))
        if out[0] == "ack":
            claimed += 1
            continue
        if case["throws"]:
            assert out == ("throw", b"buffer too short [E100]"), case["name"]
        elif case["fields"][0] == "":
            assert out == ("none",), case["name"]  # empty topic → return (message_handler.hpp:63)
        else:
            assert out[0] == "tm" and all(same(case["fields"][k], out[1][k]) for k in range(5)), case["name"]
        checked += 1
    return checked, claimed


def check_materialized_tm(cases, views):
    """The decode_tm_ref cases that succeed against strings a subject copied out of the records:
    views(records) -> one (topic, message_type, message_id, payload, headers) tuple of bytes per
    record.  The fixture's fields directly; headers are "" where the reference lost them to E100."""
    ok = [c for c in cases if not c["e100"]]
    got = views(fixture_records(ok))
    assert len(got) == len(ok)
    for case, v in zip(ok, got):
        f = case["fields"]
        assert same(f[1], v[1]) and same(f[2], v[2]) and same(f[3], v[3]), case["name"]
        assert same(f[4], v[4]) if case["headers_ok"] else v[4] == b"", case["name"]
    return len(ok)


# ------------------------------------------------------------------------------------------
# survey_probes.json
# ------------------------------------------------------------------------------------------
def probe_input(name):
    wire = T.tm_wire(F5, PROBE_TS)
    ack37 = T.ack_wire(b"msg_1", b"orders", b"corr", 1_700_000_000_000)
    return {
        "parse_ref_truncated": wire[:-8],
        "parse_wrapped_tm": T.session_wrap(wire),
        "parse_tm_cut_in_payload": wire[:50],
        "parse_template9": T.hdr_bytes(16, 9, 1, 1) + wire[8:],
        "parse_blk8": T.hdr_bytes(8, 1, 1, 1) + wire[8:],
        "parse_3_bytes": wire[:3],
        "parse_simple_ack": T.simple_ack(1_000_000_000_000),
        "decode_ack_simple": T.simple_ack(1_000_000_000_000),
        "decode_ack_exact_37": ack37,
        "decode_ack_slack8": ack37 + b"\0" * 8,
        "on_egress_tm_exact_71": wire,
        "on_egress_ack_exact_37": ack37,
    }[name]


def check_survey_probe(probe, encode, decode):
    e = probe["expect"]
    if probe["kind"] == "encode_ref":
        fields = ENCODE_PROBE_FIELDS[probe["name"]]
        (got,), (st,) = encode([fields], [PROBE_TS], T.ENC_REF_TRUNCATE8)
        if "error" in e:
            assert st == 1 and got == b""  # SBE_ENC_E109_TOPIC ↔ "topicLength too long ... [E109]"
            return
        assert len(got) == e["len"]
        if "wire_len" in e:
            assert len(encode([fields], [PROBE_TS], 0)[0][0]) == e["wire_len"]
        if "prefix_hex" in e:
            assert got.hex().startswith(e["prefix_hex"]) and got.hex().endswith(e["suffix_hex"])
        return
    rec = probe_input(probe["name"])
    if probe["kind"] == "parse":
        d = decode([rec], T.DEC_PARSE)
        pr = T.materialize_parse(rec, T.row(d, 0))
        for k, v in e.items():
            assert pr[k] == (v.encode() if isinstance(v, str) else v), (k, pr[k], v)
        return
    d = decode([rec], T.DEC_EGRESS)
    out = T.materialize_egress(rec, T.row(d, 0))
    if probe["kind"] == "decode_ack":
        assert (out[0] == "ack") == e["has"]
        if e["has"]:
            info = out[1]
            assert info["timestamp_nanos"] == e["timestamp_nanos"] and info["simple_control_ack"] == e["simple"]
            for k in ("message_id", "topic", "correlation_id"):
                if k in e:
                    assert info[k] == e[k].encode()
        return
    assert out[0] == e["outcome"]
    if e["outcome"] == "throw":
        assert out[1] == e["what"].encode()


def check_survey_probes(probes, encode, decode):
    for probe in probes:
        check_survey_probe(probe, encode, decode)
    return len(probes)


# ------------------------------------------------------------------------------------------
# lite_ref.json
# ------------------------------------------------------------------------------------------
def check_lite_encode(cases, lite_encode):
    """Each template's cases go to the subject as one batch, in fixture order."""
    checked = 0
    for t in sorted({c["template"] for c in cases}):
        sub = [c for c in cases if c["template"] == t]
        got, st = lite_encode(t, [fields_of(c["fields"]) for c in sub], [c["topic_id"] for c in sub],
                              [int(c["sequence"]) for c in sub])
        assert len(got) == len(st) == len(sub)
        for i, case in enumerate(sub):
            assert st[i] == case["status"], (t, i, st[i], case["status"])
            if st[i] == 0:
                assert same(case["record"], got[i]), (t, i)
            else:
                assert got[i] == b"", (t, i)
        checked += len(sub)
    return checked


def lite_rec(case):
    return bytes.fromhex(case["rec"])


def check_lite_decode(cases, decode):
    recs = [lite_rec(c) for c in cases]
    d = decode(recs, T.DEC_LITE)
    for i, (case, rec) in enumerate(zip(cases, recs)):
        row = T.row(d, i)
        assert tuple(int(x) for x in row["hdr"]) == struct.unpack("<4H", rec[:8]), case["name"]
        if case["e100"]:
            assert row["status"] == T.ST_LITE_E100, case["name"]
            assert not any(row["view_len"]) and not any(row["view_off"]), case["name"]
            continue
        assert row["status"] == T.ST_LITE, case["name"]
        assert int(row["ts"]) == int(case["sequence"]) and int(row["view_off"][4]) == case["topic_id"], case["name"]
        for k, fb in enumerate(case["fields"]):
            o, n = int(row["view_off"][k]), int(row["view_len"][k])
            assert same(fb, rec[o:o + n]), (case["name"], k)
    return len(cases)


# ------------------------------------------------------------------------------------------
# parse_ref.json: MessageParser::parse_message of the reference's own compiled source
# ------------------------------------------------------------------------------------------
PARSE_DEFAULTS = dict(success=False, error_message=b"", message_type=b"", message_id=b"", payload=b"", headers=b"",
                      timestamp=0, sequence_number=0, template_id=0, schema_id=0, version=0, block_length=0,
                      correlation_id=0, session_id=0, leader_member_id=0, event_code=0, leadership_term_id=0)


def pack_result(r):
    """A ParseResult dict as the fixture stores it: its fields in PARSE_DEFAULTS' order (the
    struct's, success first) without the run of default values at the end, success as 0 / 1; a
    string's bytes are the code points of the JSON string (Latin-1)."""
    vals = [r[k].decode("latin-1") if isinstance(dflt, bytes) else int(r[k]) for k, dflt in PARSE_DEFAULTS.items()]
    dflts = ["" if isinstance(d, bytes) else 0 for d in PARSE_DEFAULTS.values()]
    while vals and vals[-1] == dflts[len(vals) - 1]:
        vals.pop()
    return vals


def unpack_result(packed):
    r = dict(PARSE_DEFAULTS)
    for (k, dflt), v in zip(PARSE_DEFAULTS.items(), packed):
        r[k] = v.encode("latin-1") if isinstance(dflt, bytes) else bool(v) if isinstance(dflt, bool) else v
    return r


PARSE_COLUMNS = ["name", "rec", "pred", "desc", "result"]


def parse_ref_cases():
    """parse_ref.json's rows as dicts."""
    f = load("parse_ref.json")
    assert f["columns"] == PARSE_COLUMNS and f["result_fields"] == list(PARSE_DEFAULTS)
    return [dict(zip(PARSE_COLUMNS, row)) for row in f["cases"]]


def check_parse_ref(cases, parse):
    """parse(records) -> (parse-mode descriptors, sequence numbers, sbe_order_select's pred) of the
    subject for all records as one batch.  Every ParseResult field and the four predicates of every
    case."""
    recs = [bytes.fromhex(c["rec"]) for c in cases]
    dec, seq, pred = parse(recs)
    for i, c in enumerate(cases):
        got = T.materialize_parse(recs[i], T.row(dec, i))
        got["sequence_number"] = int(seq[i])
        exp = unpack_result(c["result"])
        assert got == exp, (c["name"], {k: (got[k], exp[k]) for k in exp if got[k] != exp[k]})
        assert int(pred[i]) == c["pred"], (c["name"], int(pred[i]), c["pred"])
    return len(cases)


def oracle_parse(recs):
    import select_lib as S
    data, off = T.pack_records(list(recs))
    dec = T.oracle_decode(data, off, T.DEC_PARSE)
    return dec, T.oracle_seq_batch(data, off, dec), S.model(data, off, dec)["pred"]


# ------------------------------------------------------------------------------------------
# the CPU subject: the oracle restatement, one record per call as the reference is called
# ------------------------------------------------------------------------------------------
def _pack(fields):
    L = np.array([[len(f) for f in fields]], np.uint32)
    arena = np.frombuffer(b"".join(fields), np.uint8) if sum(len(f) for f in fields) else np.zeros(0, np.uint8)
    return arena, L


def oracle_encode(fields_list, ts_list, flags):
    recs, sts = [], []
    for fields, ts in zip(fields_list, ts_list):
        arena, L = _pack(fields)
        out, off, st = T.oracle_encode(arena, L, np.array([ts], np.uint64), flags=flags)
        recs.append(bytes(out[int(off[0]):int(off[1])]))
        sts.append(int(st[0]))
    return recs, sts


def oracle_decode(recs, mode):
    rows = [T.oracle_decode(*T.pack_records([rec]), mode=mode) for rec in recs]
    return {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}


def oracle_lite_encode(t, fields_list, topic_ids, sequences):
    recs, sts = [], []
    for fields, tid, seq in zip(fields_list, topic_ids, sequences):
        arena, L = _pack(fields)
        out, off, st = T.oracle_encode_lite(t, arena, L, np.array([tid], np.uint32), np.array([seq], np.uint64))
        recs.append(bytes(out[int(off[0]):int(off[1])]))
        sts.append(int(st[0]))
    return recs, sts
