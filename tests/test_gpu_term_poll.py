"""GPU: sbe_term_poll against the composition of the two restatements (termscan_lib.walk for the
fragments, sbe_testlib.oracle_reassemble for the messages; tests/termpoll_lib.py), compared whole:
all six counts, msg_off[: m + 1], every message byte and the carry bytes, with out pre-filled with a
sentinel and 64 guard bytes behind carry_bytes + block_bytes - start."""
import numpy as np
import pytest

import sbe_testlib as T
import termpoll_lib as P
import termscan_lib as S

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 64


def _dev(data):
    import torch
    if len(data) == 0:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda()


def poll(codec, blk, start=0, limit=None, carry=b"", capacity=None, carry_dev=None, odd=False):
    """sbe_term_poll -> (counts, messages, carry out, result), after checking msg_off[0] and the guard."""
    import torch
    d = blk if hasattr(blk, "is_cuda") else _dev(blk)
    if carry_dev is None and len(carry):
        if odd:  # the carry at an odd address
            carry_dev = _dev(b"\0" + bytes(carry))[1:]
            assert carry_dev.data_ptr() % 2 == 1
        else:
            carry_dev = _dev(carry)
    nc = 0 if carry_dev is None else int(carry_dev.numel())
    bound = nc + int(d.numel()) - start
    out = torch.full((bound + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    r = codec.term_poll(d, start, limit, carry=carry_dev, capacity=capacity, out=out)
    torch.cuda.synchronize()
    counts = [int(x) for x in r.counts.cpu().numpy().view(np.uint64)]
    m, cb = counts[4], counts[5]
    mo = r.msg_off[: m + 1].cpu().numpy().view(np.uint64)
    o = out.cpu().numpy()
    assert int(mo[0]) == 0
    assert (o[bound:] == SENTINEL).all(), "bytes at or past carry_bytes + block_bytes - start were written"
    end = int(mo[m])
    assert end + cb <= bound
    msgs = [o[int(mo[j]):int(mo[j + 1])].tobytes() for j in range(m)]
    return counts, msgs, o[end: end + cb].tobytes(), r


def check(codec, blk, start=0, limit=None, carry=b"", capacity=None, odd=False):
    eff = limit if capacity is None else (capacity if limit is None else min(limit, capacity))
    exp = P.expect(blk, start, eff, carry)
    counts, msgs, carry_out, _ = poll(codec, blk, start, limit, carry, capacity, odd=odd)
    assert counts == exp["counts"]
    assert [len(x) for x in msgs] == [len(x) for x in exp["msgs"]]   # msg_off[: m + 1]
    assert msgs == exp["msgs"]
    assert carry_out == exp["carry"]
    return exp


@pytest.mark.parametrize("case", S.HAND_CASES, ids=[c[0] for c in S.HAND_CASES])
def test_hand_cases(codec, case):
    _, blk, start, limit, tables = case
    exp = check(codec, blk, start, limit)
    assert exp["counts"][0] == tables["fragments"] and exp["counts"][1] == tables["next"] and exp["counts"][3] == tables["stop"]
    check(codec, blk, start, limit, carry=b"open")


def test_payload_lengths_and_decoys(codec):
    check(codec, S.lengths_block())
    blk, _ = S.decoy_block()
    check(codec, blk)
    check(codec, blk, limit=5)
    check(codec, blk, limit=5, carry=P.carry_bytes(33))


def test_tile_edges(codec):
    t = codec.term_scan_tile()
    blk = S.tile_block(t)
    assert check(codec, blk)["counts"][3] == S.END
    for start in (t, t + 96, t + 32, 2 * t - 64, 7 * t - 32, 8 * t - 32):
        check(codec, blk, start)
    for limit in (1, 2, 3, 4, 5, 6, 7, 8):
        check(codec, blk, 0, limit)
    check(codec, blk, 0, None, capacity=4)
    check(codec, blk, 0, 6, capacity=3)   # frag_capacity below fragment_limit
    check(codec, blk, 0, 2, capacity=50)
    check(codec, blk, 0, 6, capacity=3, carry=b"c" * 40)


@pytest.mark.parametrize("k", range(5), ids=[name for name, _ in S.dense_blocks(1024)])
def test_tiles_packed_with_frames(codec, k):
    t = codec.term_scan_tile()
    name, blk = S.dense_blocks(t)[k]
    for start, limit in S.dense_calls(t):
        exp = check(codec, blk, start, limit)
        if name == "data32" and (start, limit) == (0, None):
            # a single, a BEGIN, a middle, an END and again: 512 empty messages per 1024-slot tile
            n = len(blk) // 32
            assert exp["counts"][0] == n and exp["counts"][4] == (n + 3) // 4 + n // 4 > 1536 and exp["counts"][2] == 0


def test_stops_in_the_first_and_in_a_later_tile(codec):
    t = codec.term_scan_tile()
    seen = set()
    for name, blk in S.stop_blocks(t):
        exp = check(codec, blk)
        seen.add((exp["counts"][3], exp["counts"][1] >= t))
        check(codec, blk, carry=b"carried")
    assert seen == {(s, later) for s in (S.SHORT, S.PARTIAL, S.UNCOMMITTED) for later in (False, True)}


def test_limit_next_to_padding(codec):
    t = codec.term_scan_tile()
    b = S.Block()
    b.frame(b"one", 0x80)
    b.pad(64)
    b.frame(b"two", 0x40)
    b.pad(96)
    b.pad_to(t + 64)
    b.frame(b"three", 0xC0)
    b.pad(32)
    b.frame(b"four", 0xC0)
    b.pad(32)
    blk = b.bytes()
    for limit, nxt in ((0, 0), (1, 64), (2, 192), (3, t + 128), (4, t + 224)):
        exp = check(codec, blk, 0, limit)
        assert exp["counts"][3] == S.LIMIT and exp["counts"][1] == nxt
        check(codec, blk, 0, limit, carry=b"zero-")
    assert check(codec, blk, 0, 5)["counts"][3] == S.END


@pytest.fixture(scope="module")
def random_block():
    return S.random_block(64 * 1024, 0x7E53)


def _shape(exp):
    """(messages with a single inside their group, multi-fragment messages) of an expectation."""
    fl = exp["walk"]["flags"]
    gapped = multi = 0
    since, singles = 0, 0   # non-single fragments and singles since the last BEGIN / END
    for f in fl:
        if f & 0xC0 == 0xC0:
            singles += since > 0   # between the group's own fragments
            continue
        if f & 0x80:
            since, singles = 0, 0
        since += 1
        if f & 0x40:
            multi += since > 1
            gapped += singles > 0
            since, singles = 0, 0
    return gapped, multi


def test_random_block(codec, random_block):
    import torch
    exp = check(codec, random_block)
    assert exp["counts"][0] == 2505 and exp["counts"][4] == 1248 and exp["counts"][5] == 0
    assert _shape(exp) == (135, 419)
    # the device chain the call replaces gives the same bytes
    d = _dev(random_block)
    s = codec.term_scan(d)
    n = int(s.counts[0].item())
    r = codec.reassemble(s.out, s.frag_off[: n + 1], s.flags[:n])
    p = codec.term_poll(d)
    torch.cuda.synchronize()
    m, cb = (int(x) for x in r.counts.cpu().numpy())
    assert [int(x) for x in p.counts.cpu().numpy()[4:]] == [m, cb]
    assert torch.equal(p.msg_off[: m + 1], r.msg_off[: m + 1])
    end = int(r.msg_off[m].item()) + cb
    assert torch.equal(p.out[:end], r.out[:end])


def test_random_block_limited_and_restarted(codec, random_block):
    """The first call stops at 1000 fragments with a message open; the second starts at its `next`
    with the carry as a view of the first call's out."""
    whole = P.expect(random_block)
    e1 = P.expect(random_block, 0, 1000)
    assert e1["counts"][4] == 490 and e1["counts"][5] == 1020 and e1["counts"][3] == S.LIMIT
    d = _dev(random_block)
    c1, m1, carry1, r1 = poll(codec, d, 0, 1000)
    assert c1 == e1["counts"] and m1 == e1["msgs"] and carry1 == e1["carry"]
    end1 = int(r1.msg_off[c1[4]].item())
    e2 = P.expect(random_block, c1[1], None, carry1)
    c2, m2, carry2, _ = poll(codec, d, c1[1], None, carry_dev=r1.out[end1: end1 + c1[5]])
    assert c2 == e2["counts"] and m2 == e2["msgs"] and carry2 == e2["carry"] == b""
    assert m1 + m2 == whole["msgs"]


def test_group_across_a_scan_block_edge(codec):
    blk = P.edge_group_block(1000)
    fl = check(codec, blk)["walk"]["flags"]
    assert fl[1000] == 0x80 and fl.index(0x40) > 1024 and 0xC0 in fl[1001:1024] and 0xC0 in fl[1025:fl.index(0x40)]
    check(codec, blk, carry=P.carry_bytes(100))            # shifted by one fragment, the carry dropped by the BEGIN
    check(codec, P.edge_group_block(999), carry=P.carry_bytes(100))
    # the carry itself open across 1024 fragments of singles, closed by the END
    b = S.Block()
    for k in range(1030):
        b.frame(P.pattern(2 + k % 3, k), 0xC0)
    b.frame(b"tail", 0x40)
    check(codec, b.bytes(), carry=P.carry_bytes(300))


def test_long_message(codec):
    t = codec.term_scan_tile()
    exp = check(codec, P.long_block(t))
    assert [len(x) for x in exp["msgs"]] == [6, 0, 200000, 5, 33]
    src = exp["walk"]["frag_src"]
    assert src[2] < t and src[-3] > 2 * t                    # it crosses tile edges
    exp = check(codec, P.long_block(t, single_inside=True))
    assert [len(x) for x in exp["msgs"]] == [6, 0, 25, 200000, 5, 33]
    limit, prefix = P.open_limit()
    exp = check(codec, P.long_block(t), 0, limit)
    # the message stays open: its first 73 frames (100 448 bytes, the first 100 000 and the rest of
    # the frame they end in) come out as the carry
    assert exp["counts"][4] == 2 and exp["counts"][5] == prefix == 100448 and exp["carry"] == P.pattern(200000, 11)[:prefix]
    check(codec, P.long_block(t), 0, limit, carry=P.carry_bytes(70000))


@pytest.mark.parametrize("n", P.CARRY_LENGTHS)
def test_carry_in(codec, n):
    carry = P.carry_bytes(n)
    got = {}
    for name, blk, start, limit in P.carry_first_blocks():
        exp = check(codec, blk, start, limit, carry, odd=(name in ("end", "single", "uncommitted")))
        got[name] = exp
    assert got["begin"]["msgs"] == [P.pattern(50, 1) + P.pattern(60, 2), P.pattern(9, 3)] and got["begin"]["carry"] == b""   # dropped
    assert got["single"]["carry"] == carry and len(got["single"]["msgs"]) == 2    # stays open, goes out again
    assert got["middle-end"]["msgs"][0][:n] == carry and len(got["middle-end"]["msgs"][0]) == n + 1376 + 33
    assert got["end"]["msgs"][0] == carry + P.pattern(31, 9)
    for name in ("start-at-end", "limit-0", "uncommitted"):
        assert got[name]["counts"][4] == 0 and got[name]["carry"] == carry and got[name]["counts"][0] == 0


def test_closed_loop_with_decode(codec):
    """300 session-framed orders in frames of 100 bytes: polled in one call and in two, the messages
    are the records and decode as the encoded batch does."""
    import torch
    arena, L, ts = T.fixed256_orders(300)
    enc, eoff, _ = T.oracle_encode_session(arena, L, ts, 1, 2)
    recs = [bytes(enc[int(eoff[i]):int(eoff[i + 1])]) for i in range(300)]
    blk = S.framed_records(recs, mtu=100, pad_every=7)
    exp = P.expect(blk)
    assert exp["msgs"] == recs and exp["carry"] == b""
    d = _dev(blk)
    c, msgs, carry, r = poll(codec, d)
    assert c == exp["counts"] and msgs == recs and carry == b""
    dec = codec.decode_batch(r.out, r.msg_off[: c[4] + 1], codec.DEC_PARSE_MESSAGE)
    torch.cuda.synchronize()
    want = T.oracle_decode(enc, eoff, T.DEC_PARSE)
    got = dec.numpy()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    limit = 3 * 100 + 1
    c1, m1, carry1, r1 = poll(codec, d, 0, limit)
    assert c1[:4] == [limit, S.walk(blk, 0, limit)["next"], S.walk(blk, 0, limit)["frag_off"][-1], S.LIMIT]
    assert c1[4] == 100 and c1[5] > 0
    end1 = int(r1.msg_off[c1[4]].item())
    c2, m2, carry2, _ = poll(codec, d, c1[1], None, carry_dev=r1.out[end1: end1 + c1[5]])
    assert c2[3] == S.END and carry2 == b"" and m1 + m2 == recs


def test_argument_errors_raise_before_any_launch(codec):
    import torch
    blk = _dev(S.lengths_block())
    n = int(blk.numel())
    out = torch.full((n + 200,), SENTINEL, dtype=torch.uint8, device="cuda")
    bad = [
        dict(start=8), dict(start=n + 32), dict(start=-32), dict(limit=-1), dict(capacity=-1),
        dict(block=blk[:-16]), dict(block=blk.cpu()), dict(block=blk.to(torch.int8)),
        dict(out=out[: n - 1]), dict(out=out.cpu()),
        dict(carry=out[10:20]), dict(carry=out[n + 100: n + 200], out=out),                 # overlaps out
        dict(carry=torch.zeros(4, dtype=torch.int32, device="cuda")),
        dict(carry=torch.zeros(100, dtype=torch.uint8, device="cuda"), out=out[: n + 99]),  # out too short with the carry
        dict(msg_off=torch.zeros(3, dtype=torch.int64, device="cuda")),
        dict(msg_off=torch.zeros(64, dtype=torch.int32, device="cuda")),
        dict(workspace=torch.zeros(64, dtype=torch.uint8, device="cuda")),
    ]
    for kw in bad:
        kw.setdefault("out", out)
        b = kw.pop("block", blk)
        with pytest.raises(codec.SbeError):
            codec.term_poll(b, **kw)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to out"
