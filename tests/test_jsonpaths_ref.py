"""CPU: sbe_json_extract_batch without a GPU.

The expected outputs are jsonpaths_lib.ref_extract: a tree-building restatement of jsoncpp's reader
(tests/jsonpaths/paths_ref.cpp) with the paths resolved on the tree by isObject / isMember /
operator[].  Its reader is a copy of the one in tests/autocommit/commit_ref.cpp, which
test_autocommit_ref.py pins to the oracle's orc_seq_eval; the copy is pinned to that one here (same
verdict, same canonical dump of the tree).  jsoncpp itself is absent: parity with the library is
unpinned.  Against the restatement run the hand table's own expectations and
the device walk of csrc/json_paths.hpp compiled for the host (tests/jsonpaths/paths_host_check.cpp),
once as a shared object and once inside a stand-alone program built with
-fsanitize=address,undefined."""
import struct
import subprocess

import numpy as np
import pytest

import jsonpaths_lib as J
import sbe_testlib as T
import test_oracle_seqnum as S

RANDOM_N, RANDOM_SEED = 9000, 0x7A75


def _bare(docs):
    return T.pack_records(docs)


@pytest.fixture(scope="module")
def hand():
    return _bare(J.hand_docs())


@pytest.fixture(scope="module")
def rnd():
    docs = J.random_docs(RANDOM_N, RANDOM_SEED)
    data, off = _bare(docs)
    sel = J.random_select(RANDOM_N, RANDOM_SEED + 1)
    return data, off, sel, J.ref_extract(data, off, None, J.HAND_PATHS, select=sel)


def test_reader_copy_matches_the_older_copy_on_hand_cases():
    docs = [d.encode() if isinstance(d, str) else d for d, _ in S.HAND_CASES] + J.hand_docs()
    parsed = 0
    for d in docs:
        new, old = J.ref_dump(d), J.pin_dump(d)
        assert new == old, d[:120]
        parsed += new[0] == 0
    assert parsed >= 60


def test_reader_copy_matches_the_older_copy_on_random_and_mangled_documents():
    verdicts = [0, 0, 0]
    for d in S._docs(0xD0C, 12000):
        new, old = J.ref_dump(d), J.pin_dump(d)
        assert new == old, d[:120]
        verdicts[new[0]] += 1
    assert verdicts[0] >= 3000 and verdicts[1] >= 1000, verdicts


def test_hand_table_counts():
    assert len(J.HAND) >= 80 and len(J.HAND_PATHS) == 16
    assert sorted({p.count(".") + 1 for p in J.HAND_PATHS}) == [1, 2, 3, 4]
    codes = {c for _, c, _, _ in J.HAND}
    assert codes == {J.OK, J.FAILED, J.STACK}
    seen = {(name.count(".") + 1, kind) for _, _, _, exp in J.HAND for name, (kind, _) in exp.items()}
    assert seen >= {(d, k) for d in range(1, 5) for k in range(1, 9)}
    assert {r for _, c, r, _ in J.HAND if c == J.OK} == {J.OBJ, J.ARR, J.STR, J.ESC, J.NUM, J.TRUE, J.FALSE, J.NULL}


def test_hand_table_restatement(hand):
    data, off = hand
    J.check_hand(J.ref_extract(data, off, None, J.HAND_PATHS), data, off)


def test_hand_table_device_logic(hand):
    data, off = hand
    got = J.chk_extract(data, off, None, J.HAND_PATHS)
    J.check_hand(got, data, off)
    J.same(got, J.ref_extract(data, off, None, J.HAND_PATHS), "hand", data, off)


def test_hand_table_one_path_at_a_time(hand):
    """Every path as a table of its own gives the column it has in the table of 16."""
    data, off = hand
    full = J.ref_extract(data, off, None, J.HAND_PATHS)
    for p, name in enumerate(J.HAND_PATHS):
        one = J.chk_extract(data, off, None, [name])
        for k in ("kind", "off", "len"):
            assert np.array_equal(one[k][:, 0], full[k][:, p]), (name, k)
        assert np.array_equal(one["doc"], full["doc"]) and np.array_equal(one["root_kind"], full["root_kind"])


def test_generator_covers_every_kind_at_every_depth_and_every_code(rnd):
    _, _, _, exp = rnd
    docs = np.bincount(exp["doc"], minlength=5)
    assert all(docs[c] >= 50 for c in range(5)), docs
    depth = np.array([p.count(".") + 1 for p in J.HAND_PATHS])
    for d in range(1, 5):
        kinds = np.bincount(exp["kind"][:, depth == d].reshape(-1), minlength=9)
        assert all(kinds[k] >= 50 for k in range(1, 9)), (d, kinds)
    roots = np.bincount(exp["root_kind"], minlength=9)
    assert roots[J.OBJ] >= 1000 and all(roots[k] >= 5 for k in range(1, 9)), roots


def test_random_documents_device_logic_matches_restatement(rnd):
    data, off, sel, exp = rnd
    J.same(J.chk_extract(data, off, None, J.HAND_PATHS, select=sel), exp, "16 paths", data, off)
    one = J.ref_extract(data, off, None, J.PATHS_1, select=sel)
    J.same(J.chk_extract(data, off, None, J.PATHS_1, select=sel), one, "1 path", data, off)
    p = J.HAND_PATHS.index(J.PATHS_1[0])
    assert np.array_equal(one["kind"][:, 0], exp["kind"][:, p]) and np.array_equal(one["off"][:, 0], exp["off"][:, p])
    assert not (exp["doc"][sel == 0] != J.NOT_SELECTED).any() and (exp["kind"][exp["doc"] != J.OK] == 0).all()


def test_seqnum_suite_documents_device_logic_matches_restatement():
    data, off = _bare(list(S._docs(0xD0C, 3000)))
    paths = ["_sequence_number", "message", "message._sequence_number", "message.message",
             "message.message.message._sequence_number"]
    J.same(J.chk_extract(data, off, None, paths), J.ref_extract(data, off, None, paths), "seqnum docs", data, off)


@pytest.mark.parametrize("view", [3, 4])
def test_views_of_decoded_records(view):
    recs = J.random_records(1500, 77 + view)
    data, off = T.pack_records(recs)
    dec = T.oracle_decode(data, off, T.DEC_PARSE)
    sel = J.random_select(len(recs), 5)
    exp = J.ref_extract(data, off, dec, J.HAND_PATHS, view=view, select=sel)
    J.same(J.chk_extract(data, off, dec, J.HAND_PATHS, view=view, select=sel), exp, f"view {view}", data, off)
    tm = dec["status"] == T.ST_TM
    assert (exp["doc"][~tm] == J.NOT_SELECTED).all() and (~tm).sum() >= 50
    assert (exp["doc"][tm & (sel != 0)] != J.NOT_SELECTED).all()
    cut = tm & ((dec["flags"] & 0x4) != 0) & (sel != 0)  # SBE_FL_HEADERS_E100
    assert cut.sum() >= 5 and (view != 4 or (exp["doc"][cut] == J.EMPTY).all())
    ok = exp["kind"] != 0  # every range lies inside its view
    vo, vl = dec["view_off"][:, view][:, None], dec["view_len"][:, view][:, None]
    assert (exp["off"] >= vo)[ok].all() and (exp["off"] + exp["len"] <= vo + vl)[ok].all() and ok.sum() > 500


def test_views_are_kept_inside_their_records():
    """Descriptors that point outside the record are clamped as sbe_commit_kernel clamps them."""
    doc = b'{"s":"v","a":{"b":1}}'
    recs = [T.tm_wire([b"t", b"X", b"m", doc, b"{}"], i) for i in range(6)]
    data, off = T.pack_records(recs)
    dec = T.oracle_decode(data, off, T.DEC_PARSE)
    dec["view_len"][1, 3] = 0xFFFFFFFF
    dec["view_off"][2, 3] = 0xFFFFFFF0
    dec["view_len"][3, 3] = len(doc) - 1
    dec["view_off"][4, 3] += 1
    dec["view_len"][4, 3] = 0x7FFFFFFF
    exp = J.ref_extract(data, off, dec, J.HAND_PATHS)
    J.same(J.chk_extract(data, off, dec, J.HAND_PATHS), exp, "clamped", data, off)
    assert list(exp["doc"]) == [J.OK, J.OK, J.EMPTY, J.FAILED, J.OK, J.OK]
    assert list(exp["root_kind"]) == [J.OBJ, J.OBJ, J.MISSING, J.MISSING, J.STR, J.OBJ]  # record 4 starts at "s"


BAD_TABLES = [
    ([], "no path"),
    (["p%d" % i for i in range(17)], "17 paths"),
    (["a.b.c.d.e"], "5 names"),
    (["a", "b", "a"], "a duplicate"),
    (["a.b", "c", "a.b"], "a duplicate at depth 2"),
    ([[b"a", b""]], "an empty name"),
    ([[b""]], "an empty name"),
    ([[b"x" * 65]], "a name of 65 bytes"),
    ([[b"%02d" % i + b"y" * 62, b"z" * 64] for i in range(8)] + ["a"], "1025 bytes of names"),
]
GOOD_TABLES = [["a"], ["p%d" % i for i in range(16)], ["a.b.c.d"], [[b"x" * 64]], ["a", "a.a", "a.a.a", "a.a.a.a"],
               [[b"%02d" % i + b"y" * 62, b"z" * 64] for i in range(8)], [[b"a.b"], "a.b"], [[b"\0"], [b"\0", b"\0"]]]


def test_path_table_limits():
    """The trie builder is the entry point's check of the table (the design caps of the issue)."""
    data, off = _bare([b'{"a":1}'])
    for table, what in BAD_TABLES:
        rc, out = J.chk_extract(data, off, None, table, rc=True)
        assert rc == -1, what
        assert out["doc"][0] == 0xEE  # nothing written
    for table in GOOD_TABLES:
        rc, out = J.chk_extract(data, off, None, table, rc=True)
        assert rc == 0 and out["doc"][0] == J.OK, table
        J.same(out, J.ref_extract(data, off, None, table), str(table)[:60])


def test_shared_prefixes_and_bytes_names():
    """Names are raw bytes: a dot, a NUL and non-ASCII bytes are part of a name; 16 paths under one prefix."""
    doc = b'{"a.b":1,"a":{"b":2},"\\u0000":{"\\u0000":"n"},"\xc3\xa9":{"x":[true]},"p":{' + \
          b",".join(b'"q%d":%d' % (i, i) for i in range(16)) + b"}}"
    data, off = _bare([doc, doc[:-1]])
    table = [[b"a.b"], "a.b", [b"\0", b"\0"], [b"\xc3\xa9", b"x"]]
    exp = J.ref_extract(data, off, None, table)
    J.same(J.chk_extract(data, off, None, table), exp)
    assert list(exp["kind"][0]) == [J.NUM, J.NUM, J.STR, J.ARR] and exp["doc"][1] == J.FAILED
    wide = ["p.q%d" % i for i in range(16)]
    exp = J.ref_extract(data, off, None, wide)
    J.same(J.chk_extract(data, off, None, wide), exp)
    assert (exp["kind"][0] == J.NUM).all() and [int(doc[o:o + ln]) for o, ln in zip(exp["off"][0], exp["len"][0])] == list(range(16))


def test_order_id_rule_of_the_restatement():
    """The callback body of examples/pubsub_reconnect_test.cpp:582-623 on the tree, against hand-derived
    answers: both branches, the uuid fill, non-strings, and everything its catch (...) swallows."""
    for payload, want in J.ORDER_ID_CASES:
        assert J.ref_order_ids(payload) == want, payload[:100]
    assert len(J.ORDER_ID_CASES) >= 30


def test_order_id_rule_from_the_nine_paths():
    """The same answers from the nine paths' kinds and ranges alone (what extract_order_ids has to
    go on), over the hand cases and 3 000 random Order-shaped payloads."""
    import random
    r = random.Random(11)
    names = [[b"message", b"message", b"uuid", b"x"], [b"message", b"message", b"order_details", b"uuid"],
             [b"client_order_id", b"order_id", b"order_details", b"message"], [b"client_order_id", b"order_id", b"x"]]

    def value(depth):
        k = r.random()
        if depth < 4 and k < (0.8 if depth < 2 else 0.4):
            return b"{" + b",".join(b'"%s":%s' % (r.choice(names[depth]), value(depth + 1))
                                    for _ in range(r.randrange(1, 4))) + b"}"
        if r.random() < 0.7:
            return r.choice([b'"id%d"' % r.randrange(9), b'"a\\u0042"'])
        return r.choice([b'""', b"7", b"null", b"[]", b"true"])

    docs = [p for p, _ in J.ORDER_ID_CASES] + [value(0) for _ in range(3000)]
    data, off = _bare(docs)
    got = J.chk_extract(data, off, None, J.ORDER_ID_PATHS)
    hits = 0
    for i, d in enumerate(docs):
        want = J.ref_order_ids(d)
        assert J.order_ids_from_fields(got, data, off, i) == want, d[:120]
        hits += want != (b"", b"")
    assert hits >= 300


def test_conversions_of_the_restatement():
    for text, want in J.CONVERT_CASES:
        assert J.ref_convert(b'{"v":%s}' % text, b"v") == want, text
    assert J.ref_convert(b'{"w":1}', b"v") == (b"", 0)  # Value::get's null for an absent member


def test_parse_commit_offset_of_the_restatement():
    for doc, want in J.OFFSET_CASES:
        got = J.ref_parse_commit_offset(doc)
        assert got[: len(want)] == want, (doc[:100], got)


def _write_case(path, data, off, dec, view, select, table, exp):
    P, depth, names, name_off = J.path_table(table)
    n = off.size - 1
    head = struct.pack("<8Q", 0x3130485441504A53, n, data.size, int(dec is not None), view, int(select is not None), P,
                       name_off.size - 1)
    parts = [data, off.astype(np.uint64)]
    if dec is not None:
        parts += [dec["status"], dec["flags"], dec["view_off"].astype(np.uint32), dec["view_len"].astype(np.uint32)]
    if select is not None:
        parts += [select.astype(np.uint8)]
    parts += [depth, name_off, names[: int(name_off[-1])]]
    parts += [exp[k] for k in J.KEYS]
    with open(path, "wb") as f:
        f.write(head)
        for p in parts:
            f.write(np.ascontiguousarray(p).tobytes())


def test_host_build_under_sanitizers(tmp_path, hand, rnd):
    """The same host build inside a stand-alone program with AddressSanitizer and UBSan: every
    record in a heap block of exactly its size, every result row of exactly P entries."""
    prog = J.make("paths_sanitize")
    files = []
    data, off = hand
    for name, table in (("hand16", J.HAND_PATHS), ("hand1", J.PATHS_1)):
        files.append(tmp_path / f"{name}.bin")
        _write_case(files[-1], data, off, None, 0, None, table, J.ref_extract(data, off, None, table))
    data, off, sel, exp = rnd
    n = 3000
    files.append(tmp_path / "rnd.bin")
    _write_case(files[-1], data[: int(off[n])], off[: n + 1], None, 0, sel[:n], J.HAND_PATHS, {k: v[:n] for k, v in exp.items()})
    recs = J.random_records(800, 9)
    data, off = T.pack_records(recs)
    dec = T.oracle_decode(data, off, T.DEC_PARSE)
    for view in (3, 4):
        files.append(tmp_path / f"view{view}.bin")
        _write_case(files[-1], data, off, dec, view, None, J.HAND_PATHS, J.ref_extract(data, off, dec, J.HAND_PATHS, view=view))
    r = subprocess.run([prog] + [str(f) for f in files], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{len(files)} cases ok" in r.stdout
