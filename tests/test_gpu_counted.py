"""GPU: the *_counted calls, which take their record count from device memory: n = min(*n_dev,
capacity).  Expected values are the uncounted calls' at a host n (their own tests pin those to the
oracle and the reference fixtures), compared byte for byte.  Every per-record output is prefilled
with 0xA5 and must keep it at record indices >= n; rec_off past n + 1 and rec_idx past n hold wrong
values that still lie inside the buffers (offsets descending within the data, indices below the
capacity), so that a kernel that reads them gives a wrong byte and never a fault.  The count is
written by a device op on the stream of the call."""
import os
import re

import numpy as np
import pytest
import torch

import commitfallback_lib as F
import commitsend_lib as C
import sbe_testlib as T
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu
CAP = 200
COUNTS = (0, 1, 63, 64, 65, 199, 200, 1000)
BLOCK_EDGE = (255, 256, 257)  # oj::kBlock, the emit's sizing block, is 256 (the append's plan block: plan_edge_counts)
NREC = 300
POISON = 0xA5
BLOCK_BYTES = 1 << 18
HDR = dict(session_id=5, stream_id=6, term_id=7, term_offset_base=4096, version=1)


def _rec(i):
    """A third of the records commit: CommitOffsetLite frames, JSON frames and host-resolved ones in turn."""
    mid = b"id-%d" % i
    if i % 3:
        return T.tm_wire([b"orders", b"SUBSCRIBE", b"s%d" % i, C.P, b"{}"], i)
    hd = [b'{"topic":"alpha"}', b'{"topic":"user-%d"}' % i, b'{"topic":12}', b'{"topic":"beta"}', b'{"topic":"gamma"}'][(i // 3) % 5]
    return T.tm_wire([b"orders", b"X", mid, C.PSEQ if i % 5 == 0 else C.P, hd], 1_000_000 + i)


def poisoned(n, dtype, shape=None):
    raw = torch.full((max(n, 1) * torch.empty(0, dtype=dtype).element_size(),), POISON, dtype=torch.uint8, device="cuda")
    t = raw.view(dtype)
    return t if shape is None else t.view(shape)


def raw_bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


def untouched(t, first):
    """Rows first.. of t still hold the poison."""
    return bool((raw_bytes(t[first:]) == POISON).all())


def dev_count(c):
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    t.add_(int(c))  # a device op on the current stream
    return t


class World:
    def __init__(self, codec):
        self.codec = codec
        recs = [_rec(i) for i in range(NREC)]
        self.data, self.off = T.pack_records(recs)
        self.d = to_dev(self.data, torch.uint8)
        self.ttab = codec.commit_topic_table(F.TOPICS, "cuda")
        self.tid = to_dev(np.asarray(F.TOPIC_IDS, np.uint32), torch.int32)
        self.itab = codec.commit_identifier_table(F.IDENTS, "cuda")
        self.dident = to_dev(np.frombuffer(F.DEFAULT_IDENT, np.uint8).copy(), torch.uint8)
        self.fb = codec.CommitFallback(self.ttab, self.dident, F.NOW, F.UUID0)
        self.ro = to_dev(self.off, torch.int64)
        self._stage = {}

    def rec_off(self, cap, n):
        """cap + 1 offsets: right up to n, then descending inside the data."""
        o = self.off[: cap + 1].copy()
        k = o.size - (n + 1)
        if k > 0:
            o[n + 1:] = (int(self.data.size) - 1 - np.arange(k, dtype=np.int64) * 3) % self.data.size
        return to_dev(o, torch.int64)

    def staged(self, n, cap_bytes=None, fb=True):
        """The uncounted calls over the first n records: decode, classify, emit."""
        key = (n, cap_bytes, fb)
        if key not in self._stage:
            c = self.codec
            ro = self.ro[: n + 1]
            seq = poisoned(n, torch.int64)
            dec = c.decode_batch(self.d, ro, mode=c.DEC_PARSE_MESSAGE, seq=seq)
            plan = c.classify_commits(self.d, ro, dec, self.ttab)
            out = torch.full((self.frames_cap,), POISON, dtype=torch.uint8, device="cuda")
            fr = c.emit_commit_offsets(self.d, ro, dec, plan, self.tid, self.itab, out=out,
                                       out_capacity=self.frames_cap if cap_bytes is None else cap_bytes,
                                       leadership_term_id=3, cluster_session_id=4, fallback=self.fb if fb else None,
                                       emit_idx=poisoned(n, torch.int64), status=poisoned(n, torch.uint8),
                                       out_off=poisoned(n + 1, torch.int64))
            torch.cuda.synchronize()
            self._stage[key] = (dec, plan, fr)
        return self._stage[key]

    @property
    def frames_cap(self):
        return self.codec.commit_fallback_output_bound(NREC, int(self.data.size) + NREC * 32, True)

    def full(self, cap):
        """Descriptors and plan of all cap records (inputs of the counted classify / emit)."""
        return self.staged(cap)


@pytest.fixture(scope="module")
def world(codec):
    return World(codec)


DEC_KEYS = ("status", "flags", "hdr", "ts", "view_off", "view_len")


def poisoned_decoded(codec, cap):
    return codec.Decoded(poisoned(cap, torch.uint8), poisoned(cap, torch.uint8), poisoned(cap * 4, torch.int16, (-1, 4)),
                         poisoned(cap, torch.int64), poisoned(cap * 5, torch.int32, (-1, 5)),
                         poisoned(cap * 5, torch.int32, (-1, 5)))


@pytest.mark.parametrize("mode", ["DEC_PARSE_MESSAGE", "DEC_ON_EGRESS", "DEC_LITE"])
@pytest.mark.parametrize("count", COUNTS)
def test_decode(world, codec, count, mode):
    mode = getattr(codec, mode)
    n = min(count, CAP)
    seq_e = poisoned(n, torch.int64)
    exp = codec.decode_batch(world.d, world.ro[: n + 1], mode=mode, seq=seq_e if mode == codec.DEC_PARSE_MESSAGE else None)
    ro = world.rec_off(CAP, n)
    for hint in (0, 100, 200, 300, 400):
        out, seq = poisoned_decoded(codec, CAP), poisoned(CAP, torch.int64)
        got = codec.decode_batch_counted(world.d, ro, dev_count(count), CAP, mode=mode, out=out, seq=seq,
                                         avg_record_bytes=hint)
        torch.cuda.synchronize()
        for k in DEC_KEYS:
            assert np.array_equal(raw_bytes(getattr(got, k)[:n]), raw_bytes(getattr(exp, k)[:n])), (k, count, hint)
            assert untouched(getattr(got, k), n), (k, count, hint)
        if mode == codec.DEC_PARSE_MESSAGE:
            assert np.array_equal(raw_bytes(seq[:n]), raw_bytes(seq_e[:n])), (count, hint)
        assert untouched(seq, n if mode == codec.DEC_PARSE_MESSAGE else 0)


def poisoned_plan(codec, cap, k):
    return codec.CommitPlan(poisoned(cap, torch.uint8), poisoned(cap, torch.uint8), poisoned(cap, torch.uint8),
                            poisoned(cap, torch.int32), poisoned(cap, torch.int32), poisoned(cap, torch.int32),
                            poisoned(k, torch.int64), poisoned(k + 2, torch.int64))


PLAN_REC = ("cm", "topic_src", "topic_kind", "topic_off", "topic_len", "topic_idx")


@pytest.mark.parametrize("count", COUNTS)
def test_classify(world, codec, count):
    n = min(count, CAP)
    _, exp, _ = world.staged(n)
    dec, _, _ = world.full(CAP)
    got = codec.classify_commits_counted(world.d, world.rec_off(CAP, n), dev_count(count), CAP, dec, world.ttab,
                                         out=poisoned_plan(codec, CAP, len(F.TOPICS)))
    torch.cuda.synchronize()
    for k in PLAN_REC:
        assert np.array_equal(raw_bytes(getattr(got, k)[:n]), raw_bytes(getattr(exp, k)[:n])), (k, count)
        assert untouched(getattr(got, k), n), (k, count)
    assert np.array_equal(raw_bytes(got.last), raw_bytes(exp.last)) and np.array_equal(raw_bytes(got.count), raw_bytes(exp.count))


def check_emit(world, codec, cap, count, fb, arrays=None, cap_bytes=None):
    """The counted emit of `count` of `cap` records against the uncounted one; returns both results."""
    n = min(count, cap)
    _, _, exp = world.staged(n, cap_bytes, fb)
    if arrays is None:
        dec, plan, _ = world.full(cap)
        ro = world.rec_off(cap, n)
    else:
        dec, plan, ro = arrays
    out = torch.full((world.frames_cap,), POISON, dtype=torch.uint8, device="cuda")
    got = codec.emit_commit_offsets_counted(world.d, ro, dev_count(count), cap, dec, plan, world.tid, world.itab, out,
                                            out_capacity=cap_bytes, leadership_term_id=3, cluster_session_id=4,
                                            fallback=world.fb if fb else None, out_off=poisoned(cap + 1, torch.int64),
                                            status=poisoned(cap, torch.uint8), emit_idx=poisoned(cap, torch.int64),
                                            totals=poisoned(3, torch.int64))
    torch.cuda.synchronize()
    tot = got.totals.cpu().numpy()
    assert np.array_equal(tot, exp.totals.cpu().numpy()), (count, tot)
    assert np.array_equal(raw_bytes(got.out_off[: n + 1]), raw_bytes(exp.out_off[: n + 1])), count
    assert np.array_equal(raw_bytes(got.status[:n]), raw_bytes(exp.status[:n])), count
    assert np.array_equal(raw_bytes(got.emit_idx[: int(tot[0])]), raw_bytes(exp.emit_idx[: int(tot[0])])), count
    assert untouched(got.out_off, n + 1) and untouched(got.status, n) and untouched(got.emit_idx, int(tot[0])), count
    assert np.array_equal(got.out.cpu().numpy(), exp.out.cpu().numpy()), count  # the poison behind the frames included
    return got, exp


@pytest.mark.parametrize("fb", [True, False])
@pytest.mark.parametrize("count", COUNTS)
def test_emit(world, codec, count, fb):
    got, _ = check_emit(world, codec, CAP, count, fb)
    if count >= 64 and fb:
        st = got.status[: min(count, CAP)].cpu().numpy()
        assert {F.EMITTED, F.EMITTED_JSON, F.HOST, F.NONE} <= set(st.tolist())


@pytest.mark.parametrize("count", BLOCK_EDGE)
def test_emit_across_a_sizing_block(world, codec, count):
    check_emit(world, codec, NREC, count, True)


def scan_second_trip_capacity():
    """The smallest capacity whose block sums take the scan workgroup a second trip:
    2 * (nblk + 1) > 4 * kScanThreads (commit_launches; the constants from the code)."""
    src = open(os.path.join(T.PKG, "csrc", "order_json.hpp")).read()
    block = int(re.search(r"constexpr uint32_t kBlock = (\d+);", src).group(1))
    threads = int(re.search(r"constexpr uint32_t kScanThreads = (\d+);", src).group(1))
    nblk = 2 * threads  # 2 * (nblk + 1) > 4 * threads
    return (nblk - 1) * block + 1


def test_emit_capacity_past_the_scans_second_trip(world, codec):
    cap, count = scan_second_trip_capacity(), 199
    assert 500_000 < cap < 600_000
    full_dec, full_plan, _ = world.full(CAP)
    # only the per-record arrays have the capacity's size: the first 200 records are the batch's
    dec = poisoned_decoded(codec, cap)
    for k in DEC_KEYS:
        getattr(dec, k)[:CAP] = getattr(full_dec, k)
    dec.seq = poisoned(cap, torch.int64)
    dec.seq[:CAP] = full_dec.seq
    plan = poisoned_plan(codec, cap, len(F.TOPICS))
    for k in PLAN_REC:
        getattr(plan, k)[:CAP] = getattr(full_plan, k)
    plan.last.copy_(full_plan.last)
    plan.count.copy_(full_plan.count)
    ro = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
    ro[: CAP + 1] = world.ro[: CAP + 1]
    got, _ = check_emit(world, codec, cap, count, True, arrays=(dec, plan, ro))
    assert int(got.totals[0]) > 0


def header(codec):
    return codec.TermHeader(**HDR)


def fresh_block():
    return torch.full((BLOCK_BYTES,), POISON, dtype=torch.uint8, device="cuda")


def check_append(codec, data, ro_exp, n, ro_got, cap, count, rec_idx=None, data_bytes=None, start=64, **kw):
    """term_append_counted against term_append over the n records of ro_exp (dense, host n)."""
    exp = codec.term_append(fresh_block(), data, ro_exp, start=start, header=header(codec), rec_tail=poisoned(n, torch.int64), **kw)
    got = codec.term_append_counted(fresh_block(), data, ro_got, dev_count(count), cap, rec_idx=rec_idx,
                                    data_bytes=data_bytes, start=start, header=header(codec),
                                    rec_tail=poisoned(cap, torch.int64), counts=poisoned(4, torch.int64), **kw)
    torch.cuda.synchronize()
    ce, cg = exp.counts.cpu().numpy(), got.counts.cpu().numpy()
    assert np.array_equal(cg, ce), (count, cg, ce)
    assert np.array_equal(got.block.cpu().numpy(), exp.block.cpu().numpy()), count
    a = int(cg[0])
    assert np.array_equal(got.rec_tail[:a].cpu().numpy(), exp.rec_tail[:a].cpu().numpy()), count
    assert untouched(got.rec_tail, n), count
    return got, exp


@pytest.mark.parametrize("cap,count", [(CAP, c) for c in COUNTS] + [(NREC, c) for c in BLOCK_EDGE])
def test_append_dense(world, codec, cap, count):
    n = min(count, cap)
    got, _ = check_append(codec, world.d, world.ro[: n + 1], n, world.rec_off(cap, n), cap, count)
    assert int(got.counts[0]) == n and int(got.counts[3]) == codec.TERM_APPEND_END


def test_append_dense_stops_as_the_base_call_does(world, codec):
    """A limit inside the batch and a block that ends inside it, at a count below the capacity."""
    n = 150
    lim = int(world.off[70]) + 64
    got, _ = check_append(codec, world.d, world.ro[: n + 1], n, world.rec_off(CAP, n), CAP, n, limit=lim)
    assert int(got.counts[3]) == codec.TERM_APPEND_LIMIT and 0 < int(got.counts[0]) < n
    small = BLOCK_BYTES - 4096 * 3
    got, _ = check_append(codec, world.d, world.ro[: n + 1], n, world.rec_off(CAP, n), CAP, n, start=small - small % 32)
    assert int(got.counts[3]) == codec.TERM_APPEND_TRIPPED


def plan_block_records():
    """kTaBlk, the records of one plan workgroup of the append (kMatBlk; the constants from the code)."""
    src = open(os.path.join(T.PKG, "csrc", "sbe_codec.hip")).read()
    ta = open(os.path.join(T.PKG, "csrc", "term_append.hpp")).read()
    assert re.search(r"constexpr uint32_t kTaBlk = kMatBlk;", ta)
    return int(re.search(r"constexpr int kMatBlk = (\d+);", src).group(1))


class Shorts:
    """2 * kTaBlk short records (0 to 40 bytes, a few of them empty): three plan blocks of the append
    at this capacity, (cap + 1 + kTaBlk - 1) / kTaBlk, the last of them wholly past every count used."""

    def __init__(self):
        self.blk = plan_block_records()
        self.cap = 2 * self.blk
        rng = np.random.default_rng(29)
        lens = rng.integers(0, 41, self.cap)
        self.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.data = rng.integers(0, 256, int(self.off[-1]), dtype=np.uint8)
        self.d = to_dev(self.data, torch.uint8)
        self.ro = to_dev(self.off, torch.int64)
        # record j of the gathered batch: a permutation of the capacity's records
        self.perm = rng.permutation(self.cap).astype(np.uint64)

    def rec_off_wrong_behind(self, n):
        o = self.off.copy()
        k = o.size - (n + 1)
        if k > 0:
            o[n + 1:] = (int(self.data.size) - 1 - np.arange(k, dtype=np.int64) * 3) % self.data.size
        return to_dev(o, torch.int64)

    def gathered(self, n):
        """(dense bytes, offsets) of records perm[:n], and perm with wrong indices behind n."""
        parts = [self.data[int(self.off[r]): int(self.off[r + 1])] for r in self.perm[:n]]
        ro = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
        idx = self.perm.copy()
        idx[n:] = (self.perm[n:][::-1] + 1) % self.cap
        return np.concatenate(parts + [np.zeros(16, np.uint8)]), ro, idx


@pytest.fixture(scope="module")
def shorts():
    return Shorts()


def plan_edge_counts():
    b = plan_block_records()
    return (b - 1, b, b + 1)


@pytest.mark.parametrize("which", range(3))
def test_append_dense_across_a_plan_block(shorts, codec, which):
    """Counts kTaBlk - 1, kTaBlk, kTaBlk + 1 of a capacity of 2 * kTaBlk: at kTaBlk the record behind the
    last (the END stop) is thread 0 of the second plan block, and the third block lies past the count."""
    count = plan_edge_counts()[which]
    assert (shorts.cap + 1 + shorts.blk - 1) // shorts.blk == 3 and count + 1 <= 2 * shorts.blk
    got, _ = check_append(codec, shorts.d, shorts.ro[: count + 1], count, shorts.rec_off_wrong_behind(count), shorts.cap, count)
    assert int(got.counts[0]) == count and int(got.counts[3]) == codec.TERM_APPEND_END


@pytest.mark.parametrize("which", range(3))
def test_append_through_rec_idx_across_a_plan_block(shorts, codec, which):
    """The same counts through a record index table (a permutation of the capacity's records, wrong
    indices behind the count): counts[2] is added up by waves of two plan blocks."""
    count = plan_edge_counts()[which]
    dense, ro, idx = shorts.gathered(count)
    exp = codec.term_append(fresh_block(), to_dev(dense, torch.uint8), to_dev(ro, torch.int64), start=64, header=header(codec),
                            rec_tail=poisoned(count, torch.int64))
    res = codec.term_append_counted(fresh_block(), shorts.d, shorts.ro, dev_count(count), shorts.cap,
                                    rec_idx=to_dev(idx, torch.int64), start=64, header=header(codec),
                                    rec_tail=poisoned(shorts.cap, torch.int64), counts=poisoned(4, torch.int64))
    torch.cuda.synchronize()
    assert np.array_equal(res.counts.cpu().numpy(), exp.counts.cpu().numpy()), count
    assert int(res.counts[0]) == count and int(res.counts[2]) == int(ro[count])
    assert np.array_equal(res.block.cpu().numpy(), exp.block.cpu().numpy()), count
    assert np.array_equal(res.rec_tail[:count].cpu().numpy(), exp.rec_tail[:count].cpu().numpy()) and untouched(res.rec_tail, count)


def test_append_through_rec_idx_stops_in_the_second_plan_block(shorts, codec):
    """A limit that the tail reaches behind record kTaBlk + 100 of kTaBlk + 500: LIMIT, with the
    payload bytes of the appended records only, added up across the plan blocks."""
    count = shorts.blk + 500
    dense, ro, idx = shorts.gathered(count)
    d, r = to_dev(dense, torch.uint8), to_dev(ro, torch.int64)
    whole = codec.term_append(fresh_block(), d, r, start=64, header=header(codec))
    torch.cuda.synchronize()
    lim = int(whole.rec_tail[shorts.blk + 100])
    exp = codec.term_append(fresh_block(), d, r, start=64, limit=lim, header=header(codec))
    res = codec.term_append_counted(fresh_block(), shorts.d, shorts.ro, dev_count(count), shorts.cap,
                                    rec_idx=to_dev(idx, torch.int64), start=64, limit=lim, header=header(codec))
    torch.cuda.synchronize()
    c = res.counts.cpu().numpy()
    assert np.array_equal(c, exp.counts.cpu().numpy()), c
    assert int(c[3]) == codec.TERM_APPEND_LIMIT and int(c[0]) == shorts.blk + 101 and int(c[2]) == int(ro[int(c[0])])
    assert np.array_equal(res.block.cpu().numpy(), exp.block.cpu().numpy())


def gathered(frames, n):
    """The emitted frames of the first n records gathered on the host: (dense bytes, offsets, record indices)."""
    g = frames.numpy()
    idx = g["emit_idx"]
    off = g["out_off"]
    out = g["out"]
    parts = [out[int(off[r]): int(off[r + 1])] for r in idx]
    dense = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    ro = np.zeros(len(parts) + 1, np.uint64)
    ro[1:] = np.cumsum([p.size for p in parts])
    return dense, ro, idx


def wrong_idx(emit_idx, t0, cap):
    """emit_idx with wrong record indices (below the capacity) behind the first t0."""
    i = emit_idx.clone()
    i[t0:] = torch.arange(cap - t0, dtype=torch.int64, device="cuda").flip(0) % cap
    return i


@pytest.mark.parametrize("count", (CAP, 65))
def test_append_emitted_frames_through_rec_idx(world, codec, count):
    n = min(count, CAP)
    fr, _ = check_emit(world, codec, CAP, count, True)
    st = fr.status[:n].cpu().numpy()
    assert {F.EMITTED, F.EMITTED_JSON, F.HOST} <= set(st.tolist()) and 0.25 < (st != F.NONE).mean() < 0.45
    dense, ro, idx = gathered(world.staged(n)[2], n)
    t0 = int(fr.totals[0])
    assert t0 == idx.size and t0 > 10
    d = to_dev(dense, torch.uint8)
    # the frame count is the emit's totals[0], still on the device
    expb = codec.term_append(fresh_block(), d, to_dev(ro, torch.int64), start=64, header=header(codec))
    gotb = codec.term_append_counted(fresh_block(), fr.out, fr.out_off, fr.totals[0:1], CAP,
                                     rec_idx=wrong_idx(fr.emit_idx, t0, CAP), start=64, header=header(codec),
                                     rec_tail=poisoned(CAP, torch.int64))
    torch.cuda.synchronize()
    assert np.array_equal(gotb.counts.cpu().numpy(), expb.counts.cpu().numpy())
    assert int(gotb.counts[0]) == t0 and int(gotb.counts[3]) == codec.TERM_APPEND_END
    assert np.array_equal(gotb.block.cpu().numpy(), expb.block.cpu().numpy())
    assert np.array_equal(gotb.rec_tail[:t0].cpu().numpy(), expb.rec_tail[:t0].cpu().numpy()) and untouched(gotb.rec_tail, t0)


def test_append_stops_at_a_frame_the_emit_call_could_not_fit(world, codec):
    """out_capacity one byte short of the last frame: SBE_CE_OVERFLOW there, BAD_RECORD in the append,
    the bytes before it those of the whole append."""
    _, _, whole = world.staged(CAP)
    total = int(whole.totals[1])
    fr, _ = check_emit(world, codec, CAP, CAP, True, cap_bytes=total - 1)
    t0 = int(fr.totals[0])
    last = int(fr.emit_idx[t0 - 1])
    assert int(fr.status[last]) == F.OVERFLOW
    dense, ro, _ = gathered(whole, CAP)
    ref = codec.term_append(fresh_block(), to_dev(dense, torch.uint8), to_dev(ro, torch.int64), start=64, header=header(codec))
    got = codec.term_append_counted(fresh_block(), fr.out, fr.out_off, fr.totals[0:1], CAP, rec_idx=fr.emit_idx,
                                    data_bytes=total - 1, start=64, header=header(codec))
    torch.cuda.synchronize()
    c = got.counts.cpu().numpy()
    tails = ref.rec_tail.cpu().numpy()
    assert int(c[0]) == t0 - 1 and int(c[3]) == codec.TERM_APPEND_BAD_RECORD and int(c[1]) == int(tails[t0 - 2])
    assert int(c[2]) == int(ro[t0 - 1])
    g, r = got.block.cpu().numpy(), ref.block.cpu().numpy()
    assert np.array_equal(g[: int(c[1])], r[: int(c[1])]) and (g[int(c[1]):] == POISON).all()


def test_append_zero_length_records_get_a_frame(world, codec):
    """Record 1 of 4 is empty (dense); through rec_idx the empty record is appended between two others."""
    off = np.array([0, int(world.off[1]), int(world.off[1]), int(world.off[2]), int(world.off[3])], np.uint64)
    pad = np.concatenate([off, [5, 3]]).astype(np.uint64)
    got, _ = check_append(codec, world.d, to_dev(off, torch.int64), 4, to_dev(pad, torch.int64), 6, 4)
    assert int(got.counts[0]) == 4 and int(got.rec_tail[1]) - int(got.rec_tail[0]) == 32
    idx = np.array([3, 1, 0, 2, 2, 2], np.uint64)  # records 3, 1 (empty), 0; wrong indices behind
    lens = [int(off[r + 1] - off[r]) for r in (3, 1, 0)]
    dense = np.concatenate([world.data[int(off[r]): int(off[r + 1])] for r in (3, 1, 0)])
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    exp = codec.term_append(fresh_block(), to_dev(dense, torch.uint8), to_dev(ro, torch.int64), start=64, header=header(codec))
    res = codec.term_append_counted(fresh_block(), world.d, to_dev(pad, torch.int64), dev_count(3), 6,
                                    rec_idx=to_dev(idx, torch.int64), start=64, header=header(codec))
    torch.cuda.synchronize()
    assert np.array_equal(res.counts.cpu().numpy(), exp.counts.cpu().numpy())
    assert np.array_equal(res.block.cpu().numpy(), exp.block.cpu().numpy())
    assert int(res.rec_tail[1]) - int(res.rec_tail[0]) == 32
