"""The decode kernel's outputs do not depend on the order its workgroups take the tiles in.  These
cases were written for a newest-first order (workgroup b decodes tile gridDim.x - 1 - b, so the
workgroup dispatched first holds the batch's last, often partial tile; measured and not kept, DESIGN
§4) and hold for any order: every case is held to the oracle (oracle_decode / oracle_seq_batch),
record by record, so a wrong tile <-> output mapping cannot pass: the generators are seeded per
record, no two tiles hold the same bytes.  The round trips decode the stream the pack kernel has
just written, under each of its store policies (kOutAux, kOutAuxKeep).

Sizes are the smallest that reach every path: one, two and many tiles with a full or partial last
tile; tiles that need a second window or the straight-from-memory parse at both ends of the
reversed order; each window shape of sbe_decode_batch_sized; and a stream decoded right after the
pack kernel wrote it, with no host synchronisation in between.
"""
import functools

import numpy as np
import pytest
import torch

import sbe_testlib as T

pytestmark = pytest.mark.gpu

KEYS = ("status", "flags", "hdr", "ts", "view_off", "view_len")
# in_bytes hints of decode_batch for a batch of n records -> the window kernel they select (by the
# average record size in_bytes / n): 0 unknown 16 KiB, <= 112 B 8 KiB, <= 204 B 15 KiB, 257-320 B
# 20 KiB, > 320 B 13 KiB
HINTS = {"none": lambda n: 0, "small": lambda n: 1, "mid": lambda n: 150 * n, "wide": lambda n: 300 * n,
         "large": lambda n: 1 << 62}
LONG = 21000   # payload bytes of a record no window holds (the widest is 20 KiB): parsed from memory
MEDIUM = 6000  # payload bytes of a record a window holds, but not beside the rest of its tile


def dev(a, dtype):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({torch.uint8: np.uint8, torch.int32: np.int32, torch.int64: np.int64}[dtype])).to("cuda")


def assert_same(got, exp, what=""):
    for k in exp:
        g, e = got[k], exp[k]
        if not np.array_equal(g, e):
            bad = np.nonzero((g != e).reshape(len(e), -1).any(1))[0]
            raise AssertionError(f"{what}{k} differs at records {bad[:10]} (tiles {np.unique(bad // 64)[:10]}): "
                                 f"got {g[bad[:3]]} expected {e[bad[:3]]}")


def check_decode(codec, data, off, mode, omode, in_bytes=0, seq=False):
    n = len(off) - 1
    exp = T.oracle_decode(data, off, omode)
    dec = codec.decode_batch(dev(data, torch.uint8), dev(np.asarray(off, np.uint64), torch.int64), mode=mode,
                             in_bytes=in_bytes, seq=True if seq else None)
    torch.cuda.synchronize()
    got = dec.numpy()
    assert all(len(got[k]) == n for k in KEYS)
    assert_same(got, exp)
    if seq:
        np.testing.assert_array_equal(dec.seq.cpu().numpy().view(np.uint64), T.oracle_seq_batch(data, off, exp))
    return exp


# ---- fixed-256 Orders: a partial tile dispatched first, the tile <-> output mapping ----

@functools.lru_cache(maxsize=None)
def fixed_stream(n):
    arena, L, ts = T.fixed256_orders(n, seed=0x0DE0 + n)
    eo, eoff, _ = T.oracle_encode(arena, L, ts)
    return eo, eoff


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 64 * 37 + 5])
def test_fixed256_parse_with_seq(codec, n):
    eo, eoff = fixed_stream(n)
    check_decode(codec, eo, eoff, codec.DEC_PARSE_MESSAGE, T.DEC_PARSE, seq=True)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 64 * 37 + 5])
def test_fixed256_egress(codec, n):
    eo, eoff = fixed_stream(n)
    check_decode(codec, eo, eoff, codec.DEC_ON_EGRESS, T.DEC_EGRESS)


# ---- mixed and variable-length records with long records in the first and the last tile ----

N_VAR = 64 * 5 + 17
# (record, payload bytes): two in the first tile, two in the last, partial one (records 320..336)
LONG_AT = ((5, LONG), (40, MEDIUM), (N_VAR - 10, LONG), (N_VAR - 3, MEDIUM))


def long_payload(i, size):
    """Printable, seeded by the record; carries a "_sequence_number" the decode launch evaluates."""
    head = b'{"_sequence_number":%d,"pad":"' % (1000 + i)
    fill = T._FILL_LUT[T.splitmix64(0xF111 + i, (size + 7) // 8).view(np.uint8)[: size - len(head) - 2]]
    fill[fill == ord('"')] = ord("'")
    return head + fill.tobytes() + b'"}'


@functools.lru_cache(maxsize=None)
def mixed_stream():
    data, off = T.mixed_records(N_VAR)
    recs = [data[int(off[i]): int(off[i + 1])].tobytes() for i in range(N_VAR)]
    for i, size in LONG_AT:
        recs[i] = T.tm_wire([b"orders", b"CREATE_ORDER", b"msg_%025d" % i, long_payload(i, size), b"{}"],
                            1_760_000_000_000_000_000 + i)
    return T.pack_records(recs)


@functools.lru_cache(maxsize=None)
def var_stream():
    arena, L, ts = T.var_orders(N_VAR)
    start = np.zeros(N_VAR + 1, np.int64)
    start[1:] = np.cumsum(L.astype(np.int64).sum(1))
    parts = [arena[start[i]: start[i + 1]].tobytes() for i in range(N_VAR)]
    L = L.copy()
    for i, size in LONG_AT:
        p0 = int(L[i, :3].sum())  # the record's strings up to its payload
        old = parts[i]
        parts[i] = old[:p0] + long_payload(i, size) + old[p0 + int(L[i, 3]):]
        L[i, 3] = size
    eo, eoff, st = T.oracle_encode(np.frombuffer(b"".join(parts), np.uint8), L, ts)
    assert not st.any()
    return eo, eoff


def test_long_records_sit_in_both_end_tiles():
    """The streams hold what the cases below rely on (no GPU needed to see it)."""
    for data, off in (mixed_stream(), var_stream()):
        ln = np.diff(off.astype(np.int64))
        assert len(ln) == N_VAR
        for tile in (ln[:64], ln[320:]):
            assert (tile > 20480).any(), "a record no window holds"
            assert ((tile > 4096) & (tile < 8192)).any(), "a record that needs a later window"
            assert tile.sum() > 20480, "the tile spans more than one window of any shape"


@pytest.mark.parametrize("hint", list(HINTS))
@pytest.mark.parametrize("stream", ["mixed", "var"])
def test_long_records_both_ends(codec, stream, hint):
    data, off = mixed_stream() if stream == "mixed" else var_stream()
    exp = check_decode(codec, data, off, codec.DEC_PARSE_MESSAGE, T.DEC_PARSE, in_bytes=HINTS[hint](N_VAR), seq=True)
    seq = T.oracle_seq_batch(data, off, exp)
    for i, _ in LONG_AT:  # the long records were decoded as TopicMessages with their key evaluated
        assert exp["status"][i] == T.ST_TM and seq[i] == 1000 + i


# ---- Lite records ----

@pytest.mark.parametrize("tmpl", [301, 201])
def test_lite(codec, tmpl):
    arena, L, tid, sq = T.lite_records(129, tmpl)
    eo, eoff, _ = T.oracle_encode_lite(tmpl, arena, L, tid, sq)
    check_decode(codec, eo, eoff, codec.DEC_LITE, T.DEC_LITE)


# ---- the stream the pack kernel has just written, no host synchronisation before the decode ----

@pytest.mark.parametrize("n", [400_000, 1_060_000])
def test_roundtrip_each_store_policy(codec, n):
    """The pack's tile loop under both store policies, decoded at once: a 102 MB stream (inside
    [kKeepMin, kKeepMax]: cache-resident stores) and one just over 256 MiB (nontemporal, as the
    small batches above)."""
    arena, L, ts = T.fixed256_orders(n, seed=0xCAC4E)
    enc = codec.encode_topic_batch(dev(arena, torch.uint8), dev(L, torch.int32), dev(ts, torch.int64))
    dec = codec.decode_batch(enc.out, enc.out_off, mode=codec.DEC_PARSE_MESSAGE)
    torch.cuda.synchronize()
    eo, eoff, est = T.oracle_encode(arena, L, ts, nthreads=8)
    assert int(eoff[-1]) == 256 * n and (96 << 20 <= 256 * n <= 256 << 20) == (n == 400_000)
    np.testing.assert_array_equal(enc.out_off.cpu().numpy().view(np.uint64), eoff)
    assert np.array_equal(enc.status.cpu().numpy(), est)
    assert np.array_equal(enc.out[: 256 * n].cpu().numpy(), eo)
    assert_same(dec.numpy(), T.oracle_decode(eo, eoff, T.DEC_PARSE, nthreads=8))


def test_roundtrip_rotating_sets_no_sync(codec):
    n, nsets, steps = 64 * 3 + 1, 3, 6
    sets = []
    for k in range(nsets):
        arena, L, ts = T.fixed256_orders(n, seed=0x5E7 + k)
        cap = codec.output_bound(n, arena.size)
        dec = codec.alloc_decoded(n, "cuda")
        for key in KEYS:  # poison: every descriptor must be written by the decode
            getattr(dec, key).fill_(-1 if getattr(dec, key).dtype != torch.uint8 else 0xEE)
        sets.append(dict(host=(arena, L, ts), a=dev(arena, torch.uint8), l=dev(L, torch.int32), t=dev(ts, torch.int64),
                         out=torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda"),
                         off=torch.full((n + 1,), -1, dtype=torch.int64, device="cuda"),
                         st=torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda"),
                         dec=dec, seq=torch.zeros(n, dtype=torch.int64, device="cuda")))
    ws = codec.alloc_workspace(n, "cuda")
    torch.cuda.synchronize()
    for k in range(steps):  # enqueue only: the decode reads what the pack launch before it wrote
        b = sets[k % nsets]
        codec.encode_topic_batch(b["a"], b["l"], b["t"], out=b["out"], out_off=b["off"], status=b["st"], workspace=ws)
        codec.decode_batch(b["out"], b["off"], mode=codec.DEC_PARSE_MESSAGE, out=b["dec"], seq=b["seq"])
    torch.cuda.synchronize()
    for k, b in enumerate(sets):
        eo, eoff, est = T.oracle_encode(*b["host"])
        np.testing.assert_array_equal(b["off"].cpu().numpy().view(np.uint64), eoff)
        np.testing.assert_array_equal(b["st"].cpu().numpy(), est)
        np.testing.assert_array_equal(b["out"][: int(eoff[-1])].cpu().numpy(), eo)
        exp = T.oracle_decode(eo, eoff, T.DEC_PARSE)
        assert_same(b["dec"].numpy(), exp, what=f"set {k}: ")
        np.testing.assert_array_equal(b["seq"].cpu().numpy().view(np.uint64), T.oracle_seq_batch(eo, eoff, exp))
