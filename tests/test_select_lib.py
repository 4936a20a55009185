"""CPU: sbe_order_select without a GPU.

The expected outputs are select_lib.model: ParseResult's predicates and classify_topic restated over
Python bytes.  Against it run the device search of csrc/order_select.hpp compiled for the host
(tests/select/select_host_check.cpp), at the kernel's window and at windows small enough to put
every needle across a window edge, once as a shared object and once inside a stand-alone program
built with -fsanitize=address,undefined; and the host mirror's ParseResult::is_*() and
classify_topic over hand-built ParseResults (tests/select/select_mirror_check.cpp)."""
import struct
import subprocess

import numpy as np
import pytest

import select_lib as S
import sbe_testlib as T

MUTATED_N, MUTATED_SEED = 3000, 0x5E1


@pytest.fixture(scope="module")
def edge():
    names, data, off, dec = S.edge_case(S.window())
    return names, data, off, dec, S.model(data, off, dec)


@pytest.fixture(scope="module")
def mutated():
    data, off, dec = S.mutated_case(MUTATED_N, MUTATED_SEED)
    return data, off, dec, S.model(data, off, dec)


def test_edge_batch_composition(edge):
    names, data, off, dec, exp = edge
    S.check_composition(names, data, off, dec, exp, S.window())


def test_mutated_batch_composition(mutated):
    data, off, dec, exp = mutated
    tm = dec["status"] == S.ST_TM
    assert tm.sum() >= 1500 and (~tm).sum() >= 500
    assert 300 <= exp["select"][tm].sum() <= tm.sum() - 300
    by_payload = sum(1 for i in np.nonzero(exp["select"])[0] if b"ORDER" not in bytes(data[int(off[i]) + 34:int(off[i]) + 46]))
    assert by_payload >= 100


@pytest.mark.parametrize("win,lead", [(None, 0), (None, 7), (4096, 15), (64, 0), (64, 9), (48, 3), (80, 12)])
def test_edge_batch_device_logic(edge, win, lead):
    names, data, off, dec, exp = edge
    S.same(S.chk_select(data, off, dec, win or S.window(), lead), exp, (win, lead), names)


def test_small_records_at_every_window_and_alignment(edge):
    """The records under 1 KiB of the edge batch, at every alignment and at a few windows."""
    names, data, off, dec, exp = edge
    keep = [i for i in range(len(names)) if off[i + 1] - off[i] < 1024]
    d2, o2 = T.pack_records([bytes(data[int(off[i]):int(off[i + 1])]) for i in keep])
    dec2 = {k: v[keep] for k, v in dec.items()}
    exp2 = S.model(d2, o2, dec2)
    S.same(exp2, {k: exp[k][keep] for k in ("pred", "select", "topic_class")}, "subset", keys=("pred", "select", "topic_class"))
    for win in (48, 64, 96, 256):
        for lead in range(16):
            S.same(S.chk_select(d2, o2, dec2, win, lead), exp2, (win, lead), [names[i] for i in keep])


@pytest.mark.parametrize("win,lead", [(None, 0), (48, 5), (112, 11)])
def test_mutated_records_device_logic(mutated, win, lead):
    data, off, dec, exp = mutated
    S.same(S.chk_select(data, off, dec, win or S.window(), lead), exp, (win, lead))


def test_null_outputs_are_not_written(edge):
    names, data, off, dec, exp = edge
    got = S.chk_select(data, off, dec, S.window(), 0, want_select=False)
    assert (got["select"] == 0xEE).all()
    S.same(got, exp, "no select", names, keys=("pred", "topic_class", "totals"))
    got = S.chk_select(data, off, dec, S.window(), 0, want_class=False)
    assert (got["topic_class"] == 0xEE).all()
    S.same(got, exp, "no class", names, keys=("pred", "select", "totals"))


def test_edited_descriptors_device_logic(edge):
    """Header ids and views the decode would not write: the type clause of is_topic_message on its
    own, the other header clauses, and views that point past their records."""
    names, data, off, dec, _ = edge
    rng = np.random.default_rng(5)
    dec = {k: v.copy() for k, v in dec.items()}
    n = len(names)
    dec["hdr"][:, 1] = rng.choice([0, 1, 2, 3], n)
    dec["hdr"][:, 2] = rng.choice([0, 1, 2, 111], n)
    exp = S.model(data, off, dec)
    assert ((exp["pred"] & 2) == 0).sum() >= 50 and {int(p) for p in exp["pred"]} >= {0, 1, 2, 6, 10, 14}
    S.same(S.chk_select(data, off, dec, S.window(), 0), exp, "hdr", names)
    S.same(S.chk_select(data, off, dec, 64, 6), exp, "hdr, small window", names)
    small = np.nonzero(off[1:] - off[:-1] < 1024)[0]
    for i in small[::3]:
        k = rng.integers(0, 5)
        dec["view_len"][i, k] = (int(dec["view_len"][i, k]) + int(rng.choice([1, 16, 40, 2 ** 31, 2 ** 32 - 1]))) & 0xFFFFFFFF
    for i in small[1::3]:
        dec["view_off"][i, rng.integers(0, 5)] = rng.choice([0, 20, 300, 2 ** 32 - 1])
    exp = S.model(data, off, dec)
    S.same(S.chk_select(data, off, dec, S.window(), 0), exp, "views", names)
    S.same(S.chk_select(data, off, dec, 48, 1), exp, "views, small window", names)


def test_unknown_statuses_give_no_predicates():
    data, off = T.pack_records([S.tm(mtype=b"CREATE_ORDER", payload=b'{"side":1}')] * 70)
    dec = T.oracle_decode(data, off, T.DEC_PARSE)
    dec["status"][:] = list(range(3, 16)) + list(range(27, 70)) + [200, 255, 32, 34, 48, 49, 50, 0, 1, 2, 16, 18, 26, 27]
    exp = S.model(data, off, dec)
    assert (exp["pred"][:56] == 0).all() and exp["pred"][63] == 10
    S.same(S.chk_select(data, off, dec, S.window(), 0), exp, "statuses")


def test_host_build_under_sanitizers(tmp_path, edge, mutated):
    prog = S.make("select_sanitize")
    names, data, off, dec, exp = edge
    files = [tmp_path / "edge.bin", tmp_path / "edge64.bin", tmp_path / "mutated.bin"]
    S.write_case(files[0], data, off, dec, exp, S.window(), 0)
    S.write_case(files[1], data, off, dec, exp, 64, 11)
    S.write_case(files[2], *mutated, 96, 5)
    r = subprocess.run([prog] + [str(f) for f in files], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "3 cases ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_model_against_the_mirror_predicates(tmp_path, edge, mutated):
    """ParseResult::is_*() and classify_topic of the host mirror, over the ParseResults of both
    batches and over header ids no decode writes."""
    prog = S.make("select_mirror_check")
    cases = []
    for data, off, dec in ((edge[1], edge[2], edge[3]), mutated[:3]):
        buf = bytes(data)
        for i in range(len(off) - 1):
            rec = buf[int(off[i]):int(off[i + 1])]
            pr = S.parse_result(rec, int(dec["status"][i]), int(dec["flags"][i]), dec["hdr"][i], dec["view_off"][i], dec["view_len"][i])
            if pr is None or len(rec) > 4096:
                continue
            o, l = S.clamped(len(rec), dec["view_off"][i][0], dec["view_len"][i][0])
            cases.append(pr + (rec[o:o + l] if dec["status"][i] == S.ST_TM else b"",))
    for t in (0, 1, 2, 3):
        for s in (0, 1, 2, 111):
            for mtype in (b"", b"ORDER", b"xTopicMessage", b"order", b"CANCEL_ORDER", b"TopicMessag"):
                for payload in (b"", b"side", b"sid", b'{"quantity":1}'):
                    cases.append((t, s, mtype, payload, b"_control" if t else b"_contro"))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for t, s, mtype, payload, topic in cases:
            f.write(struct.pack("<HHIII", t, s, len(mtype), len(payload), len(topic)) + mtype + payload + topic)
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(cases) >= 3000
    for c, g in zip(cases, got):
        pr = c[:4]
        exp = (S.PR_SESSION_EVENT * S.is_session_event(*pr) | S.PR_TOPIC_MESSAGE * S.is_topic_message(*pr) |
               S.PR_ACKNOWLEDGMENT * S.is_acknowledgment(*pr) | S.PR_ORDER_MESSAGE * S.is_order_message(*pr), S.classify_topic(c[4]))
        assert g == exp, (c[:3], c[3][:60], c[4], g, exp)
    assert len({g for g in got}) >= 10
