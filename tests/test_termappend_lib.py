"""CPU: the Python restatement of the publish side of the term-buffer framing
(tests/termappend_lib.py append) held to hand-written blocks with every byte spelled out, and to the
independent builder the term_scan tests already use (termscan_lib.framed_records / walk)."""
import numpy as np
import pytest

import termappend_lib as A
import termscan_lib as S


@pytest.mark.parametrize("case", A.HAND_CASES, ids=[c[0].name for c in A.HAND_CASES])
def test_hand_cases(case):
    c, block, appended, nxt, payload, stop, tails = case
    assert len(block) == c.block_bytes
    e = c.expect()
    assert e["block"] == block
    assert (e["appended"], e["next"], e["payload"], e["stop"], e["rec_tail"]) == (appended, nxt, payload, stop, tails)


def test_every_stop_reason_has_a_hand_case():
    assert {c[5] for c in A.HAND_CASES} == {A.END, A.LIMIT, A.TRIPPED, A.TOO_LONG, A.BAD_RECORD}


def _records(mtu, seed):
    rng = np.random.default_rng(seed)
    lens = A.edge_lengths(mtu) + [int(x) for x in rng.integers(0, 3 * mtu, 200)]
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]


@pytest.mark.parametrize("mtu", A.MTUS)
def test_exact_block_equals_the_independent_builder(mtu):
    recs = _records(mtu, mtu)
    exp = S.framed_records(recs, mtu=mtu - 32)
    assert len(exp) == A.exact_block(recs, mtu)
    got = A.append(A.sentinel(len(exp)), 0, recs, mtu=mtu)
    assert got["block"] == exp
    assert (got["appended"], got["next"], got["stop"]) == (len(recs), len(exp), A.END)
    assert got["payload"] == sum(len(r) for r in recs)
    tails, at = [], 0
    for r in recs:
        at += A.required(len(r), mtu)
        tails.append(at)
    assert got["rec_tail"] == tails


@pytest.mark.parametrize("mtu", A.MTUS)
def test_a_block_32_short_trips_and_scans_clean(mtu):
    recs = _records(mtu, 1000 + mtu)
    size = A.exact_block(recs, mtu) - 32
    got = A.append(A.sentinel(size), 0, recs, mtu=mtu)
    assert (got["appended"], got["next"], got["stop"]) == (len(recs) - 1, size, A.TRIPPED)
    w = S.walk(got["block"])
    assert (w["next"], w["stop"]) == (size, S.END)
    # BEGIN .. END runs of the fragments are the records that went in
    msgs, cur = [], b""
    for k, fl in enumerate(w["flags"]):
        part = w["payload"][w["frag_off"][k]: w["frag_off"][k + 1]]
        cur = part if fl & A.BEGIN else cur + part
        if fl & A.ENDF:
            msgs.append(cur)
    assert msgs == recs[:-1]


def test_required_matches_the_frames_written():
    for mtu in A.MTUS:
        for n in list(range(0, 4 * mtu)) + [10 * (mtu - 32), 10 * (mtu - 32) + 1]:
            assert A.required(n, mtu) == len(S.framed_records([bytes(n)], mtu=mtu - 32)), (mtu, n)


def test_shared_cases_cover_every_stop():
    stops = {c.expect()["stop"] for c in A.shared_cases()}
    assert stops == {A.END, A.LIMIT, A.TRIPPED, A.TOO_LONG, A.BAD_RECORD}
