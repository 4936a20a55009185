"""The record corpus that pins parse_message and the ParseResult predicates to the reference's own
compiled source (oracle/_ref/libsbe_ref_src.so), shared by tests/test_oracle_vs_refsrc.py,
tests/test_gpu_vs_refsrc.py and tests/golden/make_golden.py: a hand table of what randomness reaches
badly, a seeded generator, the reference's verdicts, and the two conditions that keep a comparison
over them from hiding a failure.

Class counts of the reference's verdicts on corpus() (8000 records, seed 9), all kept by the
precondition (0 pad-dependent records), measured on the CPU:

    ack_strings 1808, tm 1786, session_event 1264, err_tm_e100 859, err_embedded_schema 587,
    ack_payload_default 519, err_header 337, err_session_event 233, ack_both_default 160,
    err_session_short 150, err_unknown_type 138, err_ack_short 75, err_embedded_short 42,
    err_embedded_template 42

Of the 8167 records (167 of the hand table), 558 are order messages by the reference's predicate,
103 / 183 TopicMessages have an Orders / Control topic, and 130 have a non-zero sequence number.
"""
import functools
import os
import struct
import subprocess

import numpy as np

import sbe_testlib as T
from test_oracle_seqnum import HAND_CASES
from test_oracle_vs_ref import mutate, rand_fields

N_CORPUS, SEED = 8000, 9
MIN_PER_CLASS = 20

ERROR_CLASSES = {
    b"Failed to decode message header": "err_header",
    b"Unknown message type": "err_unknown_type",
    b"Failed to decode SessionEvent": "err_session_event",
    b"Session message too short to contain embedded message": "err_session_short",
    b"Embedded message too short": "err_embedded_short",
    b"Unknown embedded message template_id": "err_embedded_template",
    b"Unknown embedded message schema_id": "err_embedded_schema",
    b"SBE TopicMessage decoding failed": "err_tm_e100",
    b"Buffer too short for Acknowledgment message. Need at least 16 bytes, got": "err_ack_short",
}
# the 14 classes every corpus comparison must hold MIN_PER_CLASS records of
CLASSES = ("tm", "session_event", "ack_strings", "ack_payload_default", "ack_both_default") + tuple(ERROR_CLASSES.values())
NULL_EMPTY = "err_null_empty"  # length 0: the hand table's alone


def outcome_class(r) -> str:
    """The class of one reference ParseResult (dict); raises on a text parse_message cannot return."""
    if not r["success"]:
        if r["error_message"] == b"Null or empty data":
            return NULL_EMPTY
        key = r["error_message"].split(b":")[0].rstrip(b"0123456789").rstrip()
        return ERROR_CLASSES[key]
    if r["message_type"] == b"SessionEvent" and r["schema_id"] == 111:
        return "session_event"
    if r["template_id"] == 2 and r["schema_id"] == 1:
        if r["message_id"] == b"ack_%d" % (r["timestamp"] & (2**64 - 1)):
            return "ack_both_default"  # no run of 3: the payload is defaulted with the id
        return "ack_payload_default" if r["payload"] == b"SUCCESS" else "ack_strings"
    assert r["template_id"] == 1 and r["schema_id"] == 1, r
    return "tm"


# ------------------------------------------------------------------------------------------
# records
# ------------------------------------------------------------------------------------------
TOPICS = (b"orders", b"order_request_topic", b"_subscriptions", b"_ack", b"_control", b"_internal", b"order", b"_acks")
TYPES = (b"CREATE_ORDER", b"xxORDERxx", b"TopicMessage", b"CANCEL_ORDER", b"order", b"ORDE")
WORDS = (b"order_details", b"token_pair", b"quantity", b"side", b"client_order_id", b"sid", b"Side", b"quantit")


def _kind_record(rng, kind):
    f = rand_fields(rng)
    ts = int(rng.integers(0, 2**63))
    # rand_fields alone names an order in about one record of 2000 and never a known topic: give a
    # quarter of the records each a topic, a type and a payload (an Ack's second run) that the
    # predicates and classify_topic look for or just miss
    if rng.random() < 0.25:
        f[0] = TOPICS[int(rng.integers(0, len(TOPICS)))]
    if rng.random() < 0.25:
        f[1] = TYPES[int(rng.integers(0, len(TYPES)))]
    if rng.random() < 0.25:
        k = 1 if kind in (1, 3) else 3
        w = WORDS[int(rng.integers(0, len(WORDS)))]
        at = int(rng.integers(0, len(f[k]) + 1))
        f[k] = f[k][:at] + w + f[k][at:]
    if kind in (0, 2) and rng.random() < 0.15:  # a payload the _sequence_number lookup has work with
        d = HAND_CASES[int(rng.integers(0, len(HAND_CASES)))][0]
        f[3] = d.encode() if isinstance(d, str) else d
    if kind == 0:
        return T.tm_wire(f, ts)
    if kind == 1:
        return T.ack_wire(*f[:3], ts) + b"\0" * int(rng.integers(0, 12))
    if kind == 2:
        return T.session_wrap(T.tm_wire(f, ts), term=int(rng.integers(-5, 5)), session=int(rng.integers(0, 2**40)))
    if kind == 3:
        return T.session_wrap(T.ack_wire(*f[:3], ts) + b"\0" * int(rng.integers(0, 12)))
    n = int(rng.choice([0, 1, 5, 40]))
    return T.session_event(int(rng.integers(-2**62, 2**62)), int(rng.integers(0, 2**40)), int(rng.integers(0, 99)),
                           int(rng.integers(-1, 4)), int(rng.integers(-1, 7)), detail=bytes(rng.integers(0, 256, n, dtype=np.uint8)))


@functools.lru_cache(maxsize=None)
def corpus(n=N_CORPUS, seed=SEED):
    """n records cycling over bare TopicMessage, bare Ack with 0-11 bytes of slack, session-wrapped
    TopicMessage, session-wrapped Ack and SessionEvent (detail of 0 / 1 / 5 / 40 bytes) over
    rand_fields with known topics, order keywords and _sequence_number documents put into a share of
    the records, each through
    test_oracle_vs_ref.mutate, then one byte among the first 48 rewritten (probability 0.2) or the
    record cut to 1..8 bytes (0.05)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        b = bytearray(mutate(rng, _kind_record(rng, i % 5)))
        r = rng.random()
        if r < 0.2:
            b[int(rng.integers(0, min(48, len(b))))] = int(rng.integers(0, 256))
        elif r < 0.25:
            b = b[: int(rng.integers(1, 9))]
        out.append(bytes(b))
    return tuple(out)


def ack_body(body: bytes, ts=5):
    return T.hdr_bytes(8, 2, 1, 1) + struct.pack("<Q", ts) + body


@functools.lru_cache(maxsize=None)
def hand_table():
    """((name, record), ...): what the generator reaches badly."""
    f5 = [b"orders", b"CREATE_ORDER", b"msg_1", b'{"side":"BUY","_sequence_number":41}', b'{"h":2}']
    tm = T.tm_wire(f5, 0x1122334455667788)
    ack = T.ack_wire(b"msg_42", b"orders", b"corr-1", 1_700_000_000_000) + b"\0" * 3
    kinds = {"tm": tm, "ack": ack, "wtm": T.session_wrap(tm), "wack": T.session_wrap(ack),
             "sev": T.session_event(-3, 2**40, 3, 1, 2, detail=b"redirect:host:1234")}
    out = [("empty", b"")]
    for name, rec in kinds.items():
        out += [(f"{name}_len{k}", rec[:k]) for k in range(1, 17)]
        out.append((f"{name}_whole", rec))
    for blk in (0, 8, 24, 32, 65535):  # the wrapper's block_length alone decides where the embedded header is read
        for name in ("wtm", "wack"):
            out.append((f"{name}_blk{blk}", struct.pack("<H", blk) + kinds[name][2:]))
    # the Ack heuristic: run lengths around 3, the printable range's edges (a signed char: 128 and
    # 255 are negative), the number of runs
    for k in (2, 3, 4):
        out.append((f"ack_run{k}", ack_body(b"\0" + b"abcd"[:k] + b"\0")))
        out.append((f"ack_run{k}_at_end", ack_body(b"\1" + b"wxyz"[:k])))
        out.append((f"ack_run{k}_then3", ack_body(b"abcd"[:k] + b"\n" + b"pqr")))
    for e in (31, 32, 126, 127, 128, 255):
        c = bytes([e])
        out.append((f"ack_edge{e}", ack_body(c + b"xy" + c + b"\0" + b"pq" + c + b"\0" + c + c + c)))
        out.append((f"ack_edge{e}_split", ack_body(b"ab" + c + b"cd")))
    for k, body in enumerate((b"\0\1\2\x7f", b"one", b"one\0two", b"one\0two\0three", b"one\0two\0three\0four")):
        out.append((f"ack_{k}runs", ack_body(body)))
    out.append(("ack_16", T.simple_ack(1000)))
    out.append(("ack_17_nonprintable", T.simple_ack(1000) + b"\x80"))
    out.append(("ack_id_literal_success", ack_body(b"SUCCESS\0SUCCESS")))
    out.append(("wack_16", T.session_wrap(T.simple_ack(77))))
    for k in (0, 3, 7, 8):  # nothing, less than a header, a bare header behind the wrapper
        out.append((f"wrapped_{k}bytes", T.session_wrap(T.hdr_bytes(16, 1, 1, 1)[:k])))
    # SessionEvent: the detail's length prefix at, short of and past the record's end, past 10 MiB
    sev = T.session_event(1, 2, 3, 4, 0, detail=None)
    for name, pre in (("0", 0), ("at_end", 5), ("short_of_end", 4), ("past_end", 6), ("10mib", 10 * 1024 * 1024),
                      ("10mib_1", 10 * 1024 * 1024 + 1), ("max", 2**32 - 1)):
        out.append((f"sev_detail_{name}", sev + struct.pack("<I", pre) + b"abcde"))
    for k in (1, 3, 4):
        out.append((f"sev_tail{k}", sev + b"\x01\x00\x00\x00"[:k]))
    out.append(("sev_len39", sev[:39]))
    out.append(("sev_blk0", struct.pack("<H", 0) + kinds["sev"][2:]))
    # template and schema ids around 1, 2 and 111, bare and embedded
    body = tm[8:28]
    ids = [(t, s) for t in (0, 1, 2, 3) for s in (1, 111)] + [(1, 0), (1, 2), (2, 0), (2, 2), (1, 110), (1, 112), (2, 110), (2, 112)]
    for t, s in ids:
        out.append((f"ids_t{t}_s{s}", T.hdr_bytes(16, t, s, 1) + body))
    for t, s in ((0, 1), (1, 1), (2, 1), (3, 1), (1, 0), (1, 2), (2, 111)):
        out.append((f"embedded_t{t}_s{s}", T.session_wrap(T.hdr_bytes(16, t, s, 1) + body)))
    # what the predicates say of a TopicMessage that names no order, and of an Ack whose run does
    out.append(("tm_plain", T.tm_wire([b"t", b"T", b"u", b"{}", b"{}"], 3)))
    out.append(("ack_order_run", ack_body(b"msg_9\0xxquantityxx")))
    assert len({n for n, _ in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def records():
    """The hand table, then the corpus."""
    return tuple(r for _, r in hand_table()) + corpus()


# ------------------------------------------------------------------------------------------
# the reference's verdicts, and the conditions
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference():
    """(results, preds, kept): the reference's ParseResult and predicate bits of every record of
    records() with zero bytes behind it, and the indices whose result is the same with PAD_NOISE
    behind it (the precondition: the others were decided by bytes past the record)."""
    res, preds, kept = [], [], []
    for i, rec in enumerate(records()):
        r, p = T.ref_parse(rec, T.PAD_ZERO)
        if (r, p) == T.ref_parse(rec, T.PAD_NOISE):
            kept.append(i)
        res.append(r)
        preds.append(p)
    return res, preds, kept


def check_conditions():
    """At most 5 % of the records left out by the precondition; every one of the 14 outcome classes
    holds MIN_PER_CLASS kept corpus records; the reference returns no text outside the known ones
    (outcome_class raises), and 'Unknown direct message template_id' is among those it never
    returns.  Returns the class counts."""
    res, _, kept = reference()
    n, n_hand = len(res), len(hand_table())
    assert len(kept) >= 0.95 * n, (len(kept), n)
    counts = dict.fromkeys(CLASSES, 0)
    for i in kept:
        c = outcome_class(res[i])
        if i >= n_hand:
            counts[c] += 1  # NULL_EMPTY cannot occur here: the generator makes no empty record
    for r in res:
        outcome_class(r)
        assert not r["error_message"].startswith(b"Unknown direct message"), r
    assert min(counts.values()) >= MIN_PER_CLASS, counts
    assert outcome_class(res[0]) == NULL_EMPTY
    return counts


def packed():
    return T.pack_records(list(records()))


def with_seq(rec, row, seq) -> dict:
    """materialize_parse plus the separately evaluated sequence_number."""
    pr = T.materialize_parse(rec, row)
    pr["sequence_number"] = int(seq)
    return pr


def diff(got: dict, exp: dict):
    return {k: (got[k], exp[k]) for k in exp if got[k] != exp[k]}


def split(data, off):
    b = bytes(np.asarray(data, np.uint8))
    return [b[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def ref_model(recs, dec):
    """pred and topic_class of every record from the reference's own predicates and classify_topic,
    in select_lib.model's layout.  topic_class is defined for TopicMessages alone, and a ParseResult
    does not carry the topic: it is read through the descriptor's first view."""
    pred = np.array([T.ref_predicates(r) for r in recs], np.uint8)
    tc = np.zeros(len(recs), np.uint8)
    for i, r in enumerate(recs):
        if dec["status"][i] == T.ST_TM:
            o, ln = int(dec["view_off"][i][0]), int(dec["view_len"][i][0])
            tc[i] = T.ref_classify_topic(r[o:o + ln])
    return pred, tc


# ------------------------------------------------------------------------------------------
# the host mirror's lines (tests/cpp/test_parse_lines.cpp) and the reference's
# ------------------------------------------------------------------------------------------
CPP_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")


def mirror_lines(recs, mode, tmp_path):
    """test_parse_lines over recs: one line per record."""
    data, off = T.pack_records(list(recs))
    path = os.path.join(str(tmp_path), f"records_{mode}.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", len(recs), len(data)))
        f.write(np.ascontiguousarray(off, np.uint64).tobytes())
        f.write(np.ascontiguousarray(data, np.uint8).tobytes())
    subprocess.run(["make", "-s", "-C", CPP_DIR, "test_parse_lines"], check=True)
    r = subprocess.run([os.path.join(CPP_DIR, "test_parse_lines"), path, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.split("\n")
    assert lines[-1] == "" and len(lines) == len(recs) + 1, (len(lines), len(recs))
    return lines[:-1]


def same_lines(got, exp, recs, what):
    for i, (g, e) in enumerate(zip(got, exp)):
        if g != e:
            gp, ep = g.split(" "), e.split(" ")
            raise AssertionError((what, i, recs[i][:48].hex(), [(a, b) for a, b in zip(gp, ep) if a != b][:4]))
