"""GPU: sbe_term_scan against the Python restatement of the term-buffer walk (tests/termscan_lib.py),
every output array and all four counts compared whole: degenerate blocks, payload lengths around
the alignment and the MTU, payloads full of decoy headers, frames against tile edges, every stop
reason in the first and in a later tile, the limit next to padding frames, a random 2 MiB block,
and the chain scan -> reassemble -> decode with a block polled in two calls."""
import numpy as np
import pytest

import sbe_testlib as T
import termscan_lib as S

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def scan(codec, blk, start=0, limit=None, capacity=None, want_out=True, want_src=True):
    """sbe_term_scan over blk -> the dict termscan_lib.walk returns (payload / frag_src None when
    not asked for), after checking that nothing past the last payload byte of out was written."""
    import torch
    d = torch.from_numpy(np.frombuffer(blk, np.uint8).copy()).cuda() if len(blk) else torch.empty(0, dtype=torch.uint8, device="cuda")
    out = torch.full((max(len(blk) - start, 0) + 64,), SENTINEL, dtype=torch.uint8, device="cuda") if want_out else None
    r = codec.term_scan(d, start, limit, capacity=capacity, out=out, want_out=want_out, want_src=want_src)
    torch.cuda.synchronize()
    n, nxt, nbytes, stop = (int(x) for x in r.counts.cpu().numpy().view(np.uint64))
    got = dict(fragments=n, next=nxt, stop=stop, frag_off=r.frag_off[: n + 1].cpu().numpy().view(np.uint64).tolist(),
               flags=r.flags[:n].cpu().numpy().tolist(), payload=None, frag_src=None)
    assert got["frag_off"][-1] == nbytes
    if want_src:
        got["frag_src"] = r.frag_src[:n].cpu().numpy().view(np.uint32).tolist()
    if want_out:
        o = out.cpu().numpy()
        got["payload"] = o[:nbytes].tobytes()
        assert (o[nbytes:] == SENTINEL).all(), "bytes past the last payload were written"
    return got


def check(codec, blk, start=0, limit=None, capacity=None, want_out=True, want_src=True):
    eff = limit if capacity is None else (capacity if limit is None else min(limit, capacity))
    exp = S.walk(blk, start, eff)
    got = scan(codec, blk, start, limit, capacity, want_out, want_src)
    for k in ("fragments", "next", "stop", "frag_off", "flags"):
        assert got[k] == exp[k], k
    if want_src:
        assert got["frag_src"] == exp["frag_src"]
    if want_out:
        assert got["payload"] == exp["payload"]
    return exp


@pytest.mark.parametrize("case", S.HAND_CASES, ids=[c[0] for c in S.HAND_CASES])
def test_hand_cases(codec, case):
    """Degenerate blocks and small chains, against the tables written out by hand."""
    _, blk, start, limit, exp = case
    got = scan(codec, blk, start, limit)
    for k, v in exp.items():
        assert got[k] == v, k
    assert got["payload"] == S.walk(blk, start, limit)["payload"]


def test_payload_lengths(codec):
    exp = check(codec, S.lengths_block())
    assert [b - a for a, b in zip(exp["frag_off"], exp["frag_off"][1:])] == [1, 31, 32, 33, 1376, 1377]
    check(codec, S.lengths_block(), want_src=False)
    check(codec, S.lengths_block(), want_out=False)


def test_decoys_never_surface(codec):
    blk, real = S.decoy_block()
    assert check(codec, blk)["frag_src"] == real
    check(codec, blk, limit=5)
    # a block that is decoys only: the chain follows what the headers say, slot by slot
    rng = np.random.default_rng(3)
    lens = rng.choice([32, 64, 96, 0, -1, 5, 1 << 30, 0x7fffffff, 320], 4096, p=[.4, .2, .1, .005, .005, .005, .005, .005, .275])
    hdrs = S.decoys(32 * 4096, lambda j: int(lens[j]))
    for start in (0, 32, 32 * 1500, 32 * 4095):
        check(codec, hdrs, start)


def test_tile_edges(codec):
    t = codec.term_scan_tile()
    blk = S.tile_block(t)
    exp = check(codec, blk)
    assert exp["stop"] == S.END and 7 * t - 32 in exp["frag_src"] and 8 * t - 32 in exp["frag_src"]
    check(codec, blk, t)            # the frame that starts the second tile
    check(codec, blk, t + 96)       # start inside the second tile, at a frame
    check(codec, blk, t + 32)       # ... and inside a payload: whatever those bytes say
    check(codec, blk, 2 * t - 64)   # the straddling frame first
    check(codec, blk, 7 * t - 32)   # an entry slot that is the last slot of a tile
    check(codec, blk, 8 * t - 32)
    for limit in (1, 2, 3, 4, 5, 6, 7, 8):
        check(codec, blk, 0, limit)
    check(codec, blk, 0, None, capacity=4)
    check(codec, blk, 0, 6, capacity=3)   # frag_capacity below fragment_limit
    check(codec, blk, 0, 2, capacity=50)


def _dense_ids():
    return [name for name, _ in S.dense_blocks(1024)]


@pytest.mark.parametrize("k", range(5), ids=_dense_ids())
def test_tiles_packed_with_frames(codec, k):
    """Chains of up to 1023 steps inside one tile (32-byte data and padding frames, a mix with
    64-byte frames, decoys of the same lengths): more steps than the top doubling level reaches,
    with the start at 0 and mid-tile and the limit in the second half of a tile and in the last."""
    t = codec.term_scan_tile()
    name, blk = S.dense_blocks(t)[k]
    for start, limit in S.dense_calls(t):
        exp = check(codec, blk, start, limit)
        if limit is None:
            assert exp["stop"] == S.END and exp["next"] == len(blk), (name, start)
    if name == "data32":
        whole = S.walk(blk)
        assert whole["fragments"] == len(blk) // 32 and S.walk(blk, 0, t // 32 + 1)["stop"] == S.LIMIT


def test_stops_in_the_first_and_in_a_later_tile(codec):
    t = codec.term_scan_tile()
    seen = set()
    for name, blk in S.stop_blocks(t):
        exp = check(codec, blk)
        assert exp["next"] == len(blk) - 32 * 4 - 64, name
        seen.add((exp["stop"], exp["next"] >= t))
    assert seen == {(s, later) for s in (S.SHORT, S.PARTIAL, S.UNCOMMITTED) for later in (False, True)}


def test_limit_next_to_padding(codec):
    t = codec.term_scan_tile()
    b = S.Block()
    b.frame(b"one", 0x80)
    b.pad(64)
    b.frame(b"two", 0x40)
    b.pad(96)
    b.pad_to(t + 64)        # the same pattern across the tile edge
    b.frame(b"three", 0xC0)
    b.pad(32)
    b.frame(b"four", 0xC0)
    b.pad(32)
    blk = b.bytes()
    for limit, nxt in ((1, 64), (2, 192), (3, t + 128), (4, t + 224)):
        exp = check(codec, blk, 0, limit)
        assert exp["stop"] == S.LIMIT and exp["next"] == nxt   # padding before: consumed; after: not
    assert check(codec, blk, 0, 5)["stop"] == S.END
    assert check(codec, blk, 0, 0)["stop"] == S.LIMIT


@pytest.fixture(scope="module")
def random_block():
    return S.random_block(64 * 1024, 0x7E53)


@pytest.mark.parametrize("want_out,want_src", [(True, True), (True, False), (False, True)])
def test_random_block(codec, random_block, want_out, want_src):
    exp = check(codec, random_block, want_out=want_out, want_src=want_src)
    assert exp["fragments"] > 1500 and exp["stop"] == S.END and exp["next"] == len(random_block)


def test_random_block_limited_and_restarted(codec, random_block):
    exp = check(codec, random_block, 0, 1000)
    assert exp["stop"] == S.LIMIT
    rest = check(codec, random_block, exp["next"])
    assert exp["fragments"] + rest["fragments"] == S.walk(random_block)["fragments"]


def _reassemble(codec, data, frag_off, flags):
    import torch
    r = codec.reassemble(data, frag_off, flags)
    torch.cuda.synchronize()
    m, carry = (int(x) for x in r.counts.cpu().numpy())
    mo = r.msg_off.cpu().numpy()
    return r, m, carry, int(mo[m])


def test_scan_reassemble_decode_chain(codec):
    """One block polled in two calls (the first limited, the second from its `next`), each fed to
    sbe_reassemble_fragments with the carry, against one call and against the restatement's
    fragments put through the oracle reassembly; the messages decode to the framed records."""
    import torch
    arena, L, ts = T.fixed256_orders(300)
    enc, eoff, _ = T.oracle_encode_session(arena, L, ts, 1, 2)
    recs = [bytes(enc[int(eoff[i]):int(eoff[i + 1])]) for i in range(300)]
    blk = S.framed_records(recs, mtu=100, pad_every=7)
    w = S.walk(blk)
    exp_msgs, exp_carry = T.oracle_reassemble(np.frombuffer(w["payload"], np.uint8), np.array(w["frag_off"], np.uint64),
                                              np.array(w["flags"], np.uint8))
    assert exp_msgs == recs and exp_carry == b""
    d = torch.from_numpy(np.frombuffer(blk, np.uint8).copy()).cuda()

    def messages(r, m, end):
        out, mo = r.out.cpu().numpy(), r.msg_off.cpu().numpy()
        return [out[int(mo[j]):int(mo[j + 1])].tobytes() for j in range(m)]

    # one call: the tables go to reassembly as they are
    s = codec.term_scan(d)
    n = int(s.counts[0].item())
    one, m, carry, end = _reassemble(codec, s.out, s.frag_off[: n + 1], s.flags[:n])
    assert m == 300 and carry == 0 and messages(one, m, end) == recs
    dec = codec.decode_batch(one.out, one.msg_off[: m + 1], codec.DEC_PARSE_MESSAGE)
    torch.cuda.synchronize()
    exp = T.oracle_decode(enc, eoff, T.DEC_PARSE)
    got = dec.numpy()
    for k in exp:
        assert np.array_equal(got[k], exp[k]), k
    # two calls: the first stops in the middle of a message
    limit = 3 * 100 + 1
    s1 = codec.term_scan(d, 0, limit)
    c1 = s1.counts.cpu().numpy()
    assert int(c1[0]) == limit and int(c1[3]) == S.LIMIT and int(c1[1]) == S.walk(blk, 0, limit)["next"]
    r1, m1, carry1, end1 = _reassemble(codec, s1.out, s1.frag_off[: limit + 1], s1.flags[:limit])
    assert m1 == 100 and carry1 > 0
    s2 = codec.term_scan(d, int(c1[1]))
    n2, _, bytes2, stop2 = (int(x) for x in s2.counts.cpu().numpy())
    assert stop2 == S.END and limit + n2 == w["fragments"]
    data2 = torch.cat([r1.out[end1: end1 + carry1], s2.out[:bytes2]])
    off2 = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), s2.frag_off[: n2 + 1] + carry1])
    fl2 = torch.cat([torch.zeros(1, dtype=torch.uint8, device="cuda"), s2.flags[:n2]])
    r2, m2, carry2, end2 = _reassemble(codec, data2, off2, fl2)
    assert carry2 == 0 and messages(r1, m1, end1) + messages(r2, m2, end2) == recs
