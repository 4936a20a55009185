"""GPU: sbe_term_append against the Python restatement of the publish-side framing
(tests/termappend_lib.py).  Every call runs on a block filled with a sentinel, with sentinel guard
bytes in front of it and behind it, and the whole buffer is compared with the restatement's block,
so a byte written anywhere it should not be fails; all four counts and rec_tail[:appended] are
compared.  Hand cases, payload lengths around the alignment and the MTU at every source alignment,
exact / short / full blocks, the limit, every stop reason, tile edges, a random 2 MiB block in one
and in two calls, and the chain encode -> append -> scan -> reassemble -> decode."""
import numpy as np
import pytest

import sbe_testlib as T
import termappend_lib as A
import termscan_lib as S

pytestmark = pytest.mark.gpu
GUARD = 64


def dev(a, dtype):
    import torch
    a = np.array(a)  # a writable copy
    return torch.from_numpy(a.view(dtype) if a.size else np.zeros(0, dtype)).cuda()


def run(codec, c, want_tail=True):
    """The case on the device, the whole guarded buffer and every count held to the restatement."""
    import torch
    exp = c.expect()
    buf = torch.full((GUARD + c.block_bytes + GUARD,), A.SENTINEL, dtype=torch.uint8, device="cuda")
    # a tensor of its own with room behind it: a batch of empty records still has a non-null `in`
    data = torch.full((len(c.data) + 16,), 0xEE, dtype=torch.uint8, device="cuda")[: len(c.data)]
    data.copy_(dev(np.frombuffer(c.data, np.uint8), np.uint8))
    off = dev(np.asarray(c.rec_off, np.uint64), np.int64)
    n = len(c.rec_off) - 1
    tail = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
    version, session, stream, term, base = c.header
    r = codec.term_append(buf[GUARD: GUARD + c.block_bytes], data, off, c.start, c.limit, c.mtu,
                          A.MAX_LEN if c.max_message_length is None else c.max_message_length,
                          codec.TermHeader(session, stream, term, base, version), rec_tail=tail[:n], want_tail=want_tail)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().tobytes()
    want = A.sentinel(GUARD) + exp["block"] + A.sentinel(GUARD)
    if got != want:
        g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        first = int(np.flatnonzero(g != w)[0]) - GUARD
        raise AssertionError("%s: the block differs first at offset %d (%d bytes differ)" % (c.name, first, int((g != w).sum())))
    appended, nxt, payload, stop = (int(x) for x in r.counts.cpu().numpy().view(np.uint64))
    assert (appended, nxt, payload, stop) == (exp["appended"], exp["next"], exp["payload"], exp["stop"]), c.name
    t = tail.cpu().numpy()
    if want_tail:
        assert r.rec_tail.numel() == n and t[:appended].tolist() == exp["rec_tail"], c.name
        assert (t[n:] == -1).all(), "rec_tail written past its n elements"
    else:
        assert r.rec_tail is None and (t == -1).all()
    return exp


@pytest.mark.parametrize("case", A.HAND_CASES, ids=[c[0].name for c in A.HAND_CASES])
def test_hand_cases(codec, case):
    c, block, appended, nxt, payload, stop, tails = case
    exp = run(codec, c)
    assert exp["block"] == block and (exp["appended"], exp["next"], exp["stop"]) == (appended, nxt, stop)
    run(codec, c, want_tail=False)


def test_shared_cases(codec):
    for c in A.shared_cases(codec.term_append_tile()):
        run(codec, c)


@pytest.mark.parametrize("mtu", A.MTUS)
def test_lengths_at_every_source_alignment(codec, mtu):
    """Lengths around the alignment and the MTU, the source at all 16 lead-in alignments, start 0
    and not, a term_offset_base that is not 0."""
    lens = A.edge_lengths(mtu)
    for lead in range(16):
        recs = [A.rec(n, lead + k) for k, n in enumerate(lens)]
        start = 0 if lead % 2 == 0 else 32 * (1 + lead)
        hdr = A.HEADER if lead % 4 == 0 else (2, -9, 0x7fffffff, lead, 0x10000 * lead + 32)
        exp = run(codec, A.Case.of("lengths", A.exact_block(recs, mtu, start), start, recs, lead=lead, mtu=mtu, header=hdr))
        assert (exp["stop"], exp["appended"]) == (A.END, len(lens))
        # each length on its own, as the last bytes of the input: the bytewise tail of the source
        if lead in (1, 15):
            for n in lens:
                one = [A.rec(n, n)]
                run(codec, A.Case.of("single", A.exact_block(one, mtu), 0, one, lead=lead, mtu=mtu))


@pytest.mark.parametrize("mtu", A.MTUS)
def test_exact_short_and_full_blocks(codec, mtu):
    recs = [A.rec(n, k) for k, n in enumerate(A.edge_lengths(mtu))]
    size = A.exact_block(recs, mtu, 64)
    exp = run(codec, A.Case.of("exact", size, 64, recs, mtu=mtu))
    assert (exp["stop"], exp["next"]) == (A.END, size)
    exp = run(codec, A.Case.of("32 short", size - 32, 64, recs, mtu=mtu))
    assert (exp["stop"], exp["next"], exp["appended"]) == (A.TRIPPED, size - 32, len(recs) - 1)
    w = S.walk(exp["block"], 64)
    assert (w["next"], w["stop"]) == (size - 32, S.END)
    exp = run(codec, A.Case.of("start at the end", 128, 128, recs, mtu=mtu))
    assert (exp["stop"], exp["next"], exp["appended"]) == (A.TRIPPED, 128, 0)
    # against the independent builder
    assert A.Case.of("exact", size - 64, 0, recs, mtu=mtu).expect()["block"] == S.framed_records(recs, mtu=mtu - 32)


def test_limit_at_before_and_behind_a_tail(codec):
    recs = [A.rec(40, k) for k in range(5)]   # 96 bytes each
    for limit, appended in ((0, 0), (95, 1), (96, 1), (97, 2), (192, 2), (10000, 5)):
        exp = run(codec, A.Case.of("limit %d" % limit, 1024, 0, recs, limit=limit))
        assert exp["appended"] == appended and exp["stop"] == (A.LIMIT if appended < 5 else A.END)


def test_too_long_first_middle_last(codec):
    for at in (0, 2, 4):
        recs = [A.rec(101 if k == at else 100 - k, k) for k in range(5)]
        exp = run(codec, A.Case.of("too long %d" % at, 4096, 0, recs, mtu=96, max_message_length=100))
        assert (exp["appended"], exp["stop"]) == (at, A.TOO_LONG)
    # over many plan blocks: the first of several too-long records, far into the batch
    recs = [A.rec(9 if k in (2500, 2501, 4000) else k % 7, k) for k in range(4200)]
    exp = run(codec, A.Case.of("too long 2500", 1 << 18, 0, recs, mtu=64, max_message_length=8))
    assert (exp["appended"], exp["stop"]) == (2500, A.TOO_LONG)


def test_bad_records(codec):
    data, off = A.pack([A.rec(20, k) for k in range(6)])
    bad = list(off)
    bad[3], bad[4] = off[4], off[3]
    exp = run(codec, A.Case("decreasing", 2048, 0, data, bad))
    assert (exp["appended"], exp["stop"]) == (3, A.BAD_RECORD)
    past = off[:5] + [len(data) + 1, len(data) + 2]
    exp = run(codec, A.Case("past the input", 2048, 0, data, past))
    assert (exp["appended"], exp["stop"]) == (4, A.BAD_RECORD)
    exp = run(codec, A.Case("huge", 2048, 0, data, [0, 20, (1 << 64) - 1, 60]))
    assert (exp["appended"], exp["stop"]) == (1, A.BAD_RECORD)
    exp = run(codec, A.Case("first", 2048, 0, data, [len(data) + 16, len(data) + 17]))
    assert (exp["appended"], exp["stop"]) == (0, A.BAD_RECORD)


def test_no_records(codec):
    exp = run(codec, A.Case.of("n == 0", 256, 96, []))
    assert (exp["appended"], exp["next"], exp["stop"]) == (0, 96, A.END)
    run(codec, A.Case.of("n == 0, limit 0", 256, 96, [], limit=0), want_tail=False)


def test_tile_edges(codec):
    t = codec.term_append_tile()
    # frames that end exactly at the tile edge, at both MTUs; the next record starts the next tile
    for mtu in (64, 1408):
        recs = [A.rec(100, 1), None, A.rec(50, 3)]
        recs[1] = A.rec(A.length_filling(t - A.required(100, mtu), mtu), 2)
        exp = run(codec, A.Case.of("ends at the tile", t + 4096, 0, recs, lead=7, mtu=mtu))
        assert exp["rec_tail"][1] == t and exp["stop"] == A.END
    # the tile is a multiple of 32 and so is every frame's offset, so no header is cut by an edge:
    # the nearest things are a header in the last 32 bytes of a tile (its payload begins the next)
    # and a header in the first 32 of one, here of middle frames at mtu 64 and of whole records
    recs = [b"", A.rec(A.length_filling(t - 64, 64), 1), A.rec(70, 2), A.rec(3, 3)]
    exp = run(codec, A.Case.of("header against the edge", 2 * t, 0, recs, lead=3, mtu=64))
    assert exp["rec_tail"][1] == t - 32 and exp["stop"] == A.END
    recs = [A.rec(A.length_filling(t - 64, 64), 1), b"", b"", A.rec(3, 3)]
    exp = run(codec, A.Case.of("record in the last 32 bytes", 2 * t, 0, recs, lead=3, mtu=64))
    assert exp["rec_tail"][:3] == [t - 64, t - 32, t]
    # one record over more than three tiles: many frames, and few
    for mtu in (64, 1408):
        recs = [A.rec(9, 1), A.rec(3 * t, 2), A.rec(9, 3)]
        exp = run(codec, A.Case.of("3 tiles", A.exact_block(recs, mtu, 32), 32, recs, lead=11, mtu=mtu,
                                   header=(1, 7, 1001, 3, 1 << 24)))
        assert exp["stop"] == A.END and exp["appended"] == 3
    # more records in a tile than the workgroup has lanes: 0- and 1-byte records, 32 and 64 bytes each
    recs = [A.rec(k % 2 if k % 5 else 0, k) for k in range(900)]
    size = A.exact_block(recs, 1408, t - 32 * 100)
    exp = run(codec, A.Case.of("dense", size, t - 32 * 100, recs, lead=1))
    assert exp["stop"] == A.END and exp["appended"] == 900
    recs = [b""] * 1200   # 512 records a tile, the most there can be
    exp = run(codec, A.Case.of("densest", 32 * 1200 + 64, 64, recs))
    assert exp["stop"] == A.END and exp["next"] == 32 * 1200 + 64
    # a trip inside a later tile, with the padding header, and one that ends a tile
    recs = [A.rec(300, k) for k in range(200)]
    exp = run(codec, A.Case.of("trip later", 2 * t + 1000 * 32, 0, recs, mtu=96))
    assert exp["stop"] == A.TRIPPED and t < exp["rec_tail"][-1] < exp["next"]
    exp = run(codec, A.Case.of("trip at a tile's end", 2 * t, 0, recs, mtu=96))
    assert exp["stop"] == A.TRIPPED and exp["next"] == 2 * t


@pytest.fixture(scope="module")
def random_records():
    return A.random_records(6500, 0x7A11)


def test_random_block_in_one_call_and_in_two(codec, random_records):
    recs = random_records
    total = A.exact_block(recs, 1408)
    assert total > 2 << 20
    exp = run(codec, A.Case.of("one call", 2 << 20, 0, recs, lead=5, max_message_length=16 << 20))
    k = exp["appended"]
    assert exp["stop"] == A.TRIPPED and 0 < k < len(recs) and exp["next"] == 2 << 20
    rest = run(codec, A.Case.of("second term", 2 << 20, 0, recs[k:], lead=9, header=(1, 7, 1001, 4, 0)))
    assert rest["stop"] == A.END and k + rest["appended"] == len(recs)
    # the two blocks scan back to the records
    msgs = []
    for blk in (exp["block"], rest["block"][: rest["next"]]):
        w, cur = S.walk(blk), b""
        for j, fl in enumerate(w["flags"]):
            part = w["payload"][w["frag_off"][j]: w["frag_off"][j + 1]]
            cur = part if fl & A.BEGIN else cur + part
            if fl & A.ENDF:
                msgs.append(cur)
    assert msgs == recs


def test_encode_append_scan_reassemble_decode_chain(codec):
    """The device chain closed: sbe_encode_session_batch (held to the oracle) -> term_append at mtu
    128 -> term_scan -> reassemble -> decode_batch; the reassembled bytes are the encoder's output
    and the decode is the oracle's decode of it."""
    import torch
    n = 300
    arena, L, ts = T.fixed256_orders(n)
    enc, eoff, _ = T.oracle_encode_session(arena, L, ts, 1, 2)
    e = codec.encode_session_batch(dev(arena, np.uint8), dev(np.asarray(L, np.uint32).reshape(-1, 5), np.int32),
                                   dev(np.asarray(ts, np.uint64), np.int64), 1, 2, flags=0)  # whole wire records, as the oracle's default
    torch.cuda.synchronize()
    goff = e.out_off.cpu().numpy().view(np.uint64)
    assert np.array_equal(goff[: n + 1], eoff[: n + 1]) and np.array_equal(e.out[: int(eoff[n])].cpu().numpy(), enc)
    size = sum(A.required(int(eoff[i + 1] - eoff[i]), 128) for i in range(n))
    block = torch.full((size,), A.SENTINEL, dtype=torch.uint8, device="cuda")
    a = codec.term_append(block, e.out, e.out_off[: n + 1], mtu=128, max_message_length=1 << 20,
                          header=codec.TermHeader(7, 1001, 3, 0, 1))
    appended, nxt, payload, stop = (int(x) for x in a.counts.cpu().numpy())
    assert (appended, nxt, payload, stop) == (n, size, int(eoff[n]), A.END)
    recs = [bytes(enc[int(eoff[i]):int(eoff[i + 1])]) for i in range(n)]
    assert block.cpu().numpy().tobytes() == S.framed_records(recs, mtu=96)
    s = codec.term_scan(block)
    c = s.counts.cpu().numpy()
    nf = int(c[0])
    assert int(c[1]) == size and int(c[3]) == S.END and int(c[2]) == int(eoff[n])
    r = codec.reassemble(s.out, s.frag_off[: nf + 1], s.flags[:nf])
    torch.cuda.synchronize()
    m, carry = (int(x) for x in r.counts.cpu().numpy())
    assert (m, carry) == (n, 0)
    assert np.array_equal(r.msg_off[: n + 1].cpu().numpy().view(np.uint64), eoff[: n + 1])
    assert np.array_equal(r.out[: int(eoff[n])].cpu().numpy(), enc)
    dec = codec.decode_batch(r.out, r.msg_off[: m + 1], codec.DEC_PARSE_MESSAGE)
    torch.cuda.synchronize()
    exp = T.oracle_decode(enc, eoff, T.DEC_PARSE)
    got = dec.numpy()
    for k in exp:
        assert np.array_equal(got[k], exp[k]), k
