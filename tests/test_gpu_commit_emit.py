"""GPU: sbe_emit_commit_offsets, the CommitOffsetLite frames of the records sbe_classify_commits
committed, compacted on the device.  Every output (out, out_off, status, emit_idx, totals) is
compared byte for byte and element for element with commitsend_lib.ref_emit: the restated plan
(autocommit_lib.ref_classify), the oracle's template-301 encoder and its session header bytes.
The decode and classify outputs the call consumes are the device's own."""
import ctypes

import numpy as np
import pytest
import torch

import autocommit_lib as A
import commitsend_lib as C
import contract_lib as G
import sbe_testlib as T
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu
SENTINEL = 0xEE
POISON_I64 = C.POISON - 2**64


class Dev:
    """A batch on the device: decoded (seq pre-filled with a poison) and classified there."""

    def __init__(self, codec, recs, lead=0, topics=C.TOPICS, ids=C.TOPIC_IDS, idents=C.IDENTS):
        self.codec, self.topics, self.ids, self.idents = codec, topics, ids, idents
        self.data, self.off, self.dec, self.seq = C.batch(recs, lead)
        self.n = self.off.size - 1
        self.plan = A.ref_classify(self.data, self.off, self.dec, topics)
        self.d = to_dev(self.data if self.data.size else np.zeros(16, np.uint8), torch.uint8)
        self.ro = to_dev(self.off.astype(np.uint64), torch.int64)
        seq = torch.full((max(self.n, 1),), POISON_I64, dtype=torch.int64, device="cuda")
        self.gdec = codec.decode_batch(self.d, self.ro, mode=codec.DEC_PARSE_MESSAGE, seq=seq)
        self.gplan = codec.classify_commits(self.d, self.ro, self.gdec, topics)
        self.tid = to_dev(np.asarray(ids, np.uint32), torch.int32)
        self.itab = codec.commit_identifier_table(idents, "cuda")

    def expected(self, use_seq=True, **kw):
        return C.ref_emit(self.data, self.off, self.dec, self.plan, self.ids, self.idents,
                          seq=self.seq if use_seq else None, **kw)

    def run(self, use_seq=True, mask=None, flags=0, session=True, term=0, sess=0, cap=None, out_shift=0):
        """The call through the binding into a sentinel-filled `out` at base + out_shift; returns the
        outputs as numpy (out: the whole buffer, sentinel tail included)."""
        exp_total = int(self.expected(use_seq, mask=mask, flags=flags, session=session)["out_off"][-1])
        cap = exp_total if cap is None else cap
        raw = torch.full((cap + out_shift + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        dec = self.gdec
        if not use_seq:
            dec = self.codec.Decoded(dec.status, dec.flags, dec.hdr, dec.ts, dec.view_off, dec.view_len, None)
        m = None if mask is None else to_dev(np.asarray(mask, np.uint8), torch.uint8)
        r = self.codec.emit_commit_offsets(self.d, self.ro, dec, self.gplan, self.tid, self.itab, mask=m, flags=flags,
                                           session=session, leadership_term_id=term, cluster_session_id=sess,
                                           out=raw[out_shift:], out_capacity=cap)
        torch.cuda.synchronize()
        got = r.numpy()
        assert (raw[:out_shift].cpu().numpy() == SENTINEL).all()
        return got

    def check(self, what="", **kw):
        exp = self.expected(**{k: v for k, v in kw.items() if k != "out_shift"})
        got = self.run(**kw)
        C.same(got, exp, what)
        tail = got["out"][exp["out"].size:]
        assert (tail == SENTINEL).all(), (what, "bytes written past the last frame that fits", np.nonzero(tail != SENTINEL)[0][:5])
        return got, exp


def _rec(i, emit, long_id=None):
    if not emit:
        return T.tm_wire([b"orders", b"SUBSCRIBE", b"s%d" % i, C.P, b"{}"], i)
    hd = [b"{}", b'{"topic":"alpha"}', b'{"topic":"beta"}', b'{"topic":""}'][i % 4]
    pl = C.PSEQ if i % 3 == 0 else C.P
    return T.tm_wire([b"orders", b"X", long_id if long_id is not None else b"id-%d" % i, pl, hd], i)


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "last_tile"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 4096 + 7])
def test_small_shapes(codec, n, pattern):
    first_of_last = (n - 1) // 64 * 64
    emit = {"all": lambda i: True, "none": lambda i: False, "alternating": lambda i: i % 2 == 1,
            "last_tile": lambda i: i >= first_of_last}[pattern]
    b = Dev(codec, [_rec(i, emit(i)) for i in range(n)])
    got, exp = b.check((n, pattern), term=3, sess=4)
    want = sum(1 for i in range(n) if emit(i))
    assert int(got["totals"][0]) == want and (got["status"] == C.EMITTED).sum() == want


@pytest.mark.parametrize("lead", [0, 7])
@pytest.mark.parametrize("use_seq", [True, False])
def test_hand_table_covers_every_status(codec, lead, use_seq):
    """Every status but OVERFLOW, the ids of 65534 (emits) and 65535 bytes (E109, 0 bytes), and the
    sequence rule: unflagged records carry 0 though seq holds a poison there; seq == NULL: 0 everywhere."""
    b = Dev(codec, C.hand_records(), lead=lead)
    got, exp = b.check(("hand", lead), use_seq=use_seq, term=-1, sess=2**62)
    assert list(got["status"]) == list(C.hand_status())
    seqs = [int.from_bytes(bytes(got["out"][int(got["out_off"][i]) + 44: int(got["out_off"][i]) + 52]), "little")
            for i in got["emit_idx"]]
    assert sorted(set(seqs)) == ([0, 123456789012] if use_seq else [0])
    assert (b.gdec.seq.cpu().numpy().view(np.uint64) == C.POISON).any()


@pytest.mark.parametrize("session", [True, False])
def test_long_ids(codec, session):
    """Ids longer than the writing launch's LDS window (5000 and 9000 bytes among short ones, then
    65534) go straight from the input to the frame; 65535 is E109."""
    longs = {5: 5000, 70: 9000, 71: 65534, 100: 65535, 130: 4000}
    recs = [_rec(i, True, long_id=bytes([65 + i % 26]) * longs[i] if i in longs else None) for i in range(140)]
    b = Dev(codec, recs, lead=3)
    got, exp = b.check("long", session=session, term=9, sess=8)
    assert got["status"][100] == C.E109 and got["out_off"][101] == got["out_off"][100]
    assert (np.delete(got["status"], 100) == C.EMITTED).all()


@pytest.mark.parametrize("out_shift", [0, 5])
@pytest.mark.parametrize("lead", [0, 7])
@pytest.mark.parametrize("session", [True, False])
def test_alignment_sweep(codec, session, lead, out_shift):
    """Id lengths 1..48 and identifier lengths 0..17; every tile's bytes are 1 mod 16, so the output
    bases of the 18 tiles take every residue mod 16."""
    topics = [b"orders"] + [b"t%d" % j for j in range(1, 18)]
    idents = [b"I" * j for j in range(18)]
    ids = list(range(100, 118))
    recs, tiles = [], 18
    for t in range(tiles):
        tile_bytes = 0
        for r in range(64):
            i, j = 64 * t + r, (64 * t + r) % 18
            idn = 1 + (i * 7 + t) % 48
            if r == 63:  # 24 (+ 32) bytes of framing per record are 0 mod 16 over a tile of 64
                idn = 1 + (1 - tile_bytes - j - 1) % 16
                idn += 16 * (t % 3)
            tile_bytes += idn + j
            hd = b"{}" if j == 0 else b'{"topic":"t%d"}' % j
            recs.append(T.tm_wire([b"orders", b"X", bytes([97 + i % 26]) * idn, C.P, hd], i))
    recs += [T.tm_wire([b"orders", b"X", b"tail-%d" % i, C.P, b'{"topic":"t%d"}' % (i + 1)], i) for i in range(5)]
    b = Dev(codec, recs, lead=lead, topics=topics, ids=ids, idents=idents)
    got, exp = b.check(("sweep", session, lead, out_shift), session=session, term=1, sess=2, out_shift=out_shift)
    assert {int(exp["out_off"][64 * t]) % 16 for t in range(tiles)} == set(range(16))
    idl = b.dec["view_len"][:, 2]
    assert set(range(1, 49)) <= set(int(x) for x in idl) and (got["status"] == C.EMITTED).all()


@pytest.fixture(scope="module")
def rnd(codec):
    return Dev(codec, C.random_records(), lead=5)


def test_random_batch(rnd):
    got, exp = rnd.check("random", term=0x0102030405060708, sess=-2)
    cnt = np.bincount(got["status"], minlength=5)
    assert all(cnt[s] >= 1 for s in (C.NONE, C.EMITTED, C.HOST, C.E109)) and cnt[C.EMITTED] * 10 >= rnd.n, cnt
    # the device's own plan is the restated one, so the composition above describes this call
    gp = rnd.gplan.numpy()
    assert np.array_equal(gp["cm"], rnd.plan["cm"]) and np.array_equal(gp["topic_idx"], rnd.plan["topic_idx"])


def test_mask_and_last_only(codec, rnd):
    mask = (np.arange(rnd.n) % 3 != 1).astype(np.uint8)
    got, _ = rnd.check("mask", mask=mask, term=7, sess=7)
    assert (got["status"][mask == 0] == C.NONE).all()
    got, _ = rnd.check("last_only", flags=C.LAST_ONLY, term=7, sess=7)
    k = len(C.TOPICS)
    assert 2 <= int(got["totals"][0]) <= k
    assert not (rnd.plan["topic_idx"] == 3).any() and rnd.plan["last"][3] == 2**64 - 1  # the duplicate entry
    with pytest.raises(codec.SbeError, match="EINVAL"):
        rnd.run(flags=C.LAST_ONLY, mask=mask)


@pytest.mark.parametrize("which", ["minus1", "mid", "zero"])
def test_capacity(codec, rnd, which):
    """out_off and totals describe the full layout whatever the capacity; nothing is written at or
    past the end of the last frame that fits (a sentinel follows the capacity)."""
    full = rnd.expected(term=1, sess=1)
    total = int(full["out_off"][-1])
    cap = {"minus1": total - 1, "mid": int(full["out_off"][rnd.n // 2]) + 5, "zero": 0}[which]
    if which == "zero":  # out = NULL sizes the batch
        r = codec.emit_commit_offsets(rnd.d, rnd.ro, rnd.gdec, rnd.gplan, rnd.tid, rnd.itab, leadership_term_id=1,
                                      cluster_session_id=1, out=None, out_capacity=0)
        torch.cuda.synchronize()
        got = r.numpy()
        assert got["out"] is None
        got["out"] = np.zeros(0, np.uint8)
        C.same(got, rnd.expected(term=1, sess=1, cap=0), which)
    else:
        got, exp = rnd.check(which, term=1, sess=1, cap=cap)
        assert (got["status"] == C.OVERFLOW).any() and (got["status"] == C.EMITTED).any()
    assert np.array_equal(got["out_off"], full["out_off"]) and np.array_equal(got["totals"], full["totals"])
    assert np.array_equal(got["emit_idx"], full["emit_idx"])


def test_fused_equals_unfused(codec, rnd):
    """out equals sbe_encode_lite_batch on the gathered strings with session headers inserted."""
    exp = rnd.expected(term=11, sess=12)
    got = rnd.run(term=11, sess=12)
    sel = [int(i) for i in exp["emit_idx"]]
    strs, tid, sq = [], [], []
    for i in sel:
        j = int(rnd.plan["topic_idx"][i])
        b = int(rnd.off[i]) + int(rnd.dec["view_off"][i, 2])
        strs.append((bytes(rnd.data[b: b + int(rnd.dec["view_len"][i, 2])]), C.IDENTS[j]))
        tid.append(C.TOPIC_IDS[j])
        flagged = rnd.dec["flags"][i] & (T.FL_SEQ_KEY | T.FL_SEQ_ESC)
        sq.append(int(rnd.seq[i]) if flagged else 0)
    arena = np.frombuffer(b"".join(a + b for a, b in strs), np.uint8)
    L = np.array([[len(a), len(b)] for a, b in strs], np.uint32)
    enc = codec.encode_lite_batch(codec.COMMIT_OFFSET_LITE, to_dev(arena, torch.uint8), to_dev(L, torch.int32),
                                  to_dev(np.array(tid, np.uint32), torch.int32), to_dev(np.array(sq, np.uint64), torch.int64))
    torch.cuda.synchronize()
    lo = enc.out_off.cpu().numpy().view(np.uint64)
    lite = enc.out.cpu().numpy()
    hdr = C.session_header(11, 12).tobytes()
    unfused = b"".join(hdr + lite[int(lo[r]): int(lo[r + 1])].tobytes() for r in range(len(sel)))
    assert got["out"][: len(unfused)].tobytes() == unfused and int(got["totals"][1]) == len(unfused)


# ------------------------------------------------------------------------------------------
# the call contract (include/sbecodec.h), through the C ABI with every buffer the test's
# ------------------------------------------------------------------------------------------
def _raw(codec, b, run, n=None, cap=None, mask=None, flags=0, session=1, k=None, out=True, shifts=None, null=()):
    """sbe_emit_commit_offsets with outputs from `run` at their minimal alignment.  shifts: extra
    byte offsets on named pointers (a misaligned array); null: pointers passed as NULL."""
    n = b.n if n is None else n
    shifts = shifts or {}
    full = int(b.expected()["out_off"][-1])
    cap = full if cap is None else cap
    m = max(b.n, 1)
    bufs = dict(out_off=run.buf("out_off", b.n + 1, torch.int64), status=run.buf("status", m, torch.uint8),
                emit_idx=run.buf("emit_idx", m, torch.int64), totals=run.buf("totals", 3, torch.int64),
                out=run.buf("out", full + 32, torch.uint8, align=1),
                ws=run.buf("ws", codec.commit_emit_workspace_size(b.n), torch.uint8, align=16))

    def p(name, t):
        if name in null or t is None:
            return None
        return ctypes.c_void_p(t.data_ptr() + shifts.get(name, 0))

    gd = b.gdec
    d = codec._Decoded(p("status_in", gd.status), p("flags_in", gd.flags), p("hdr", gd.hdr), p("ts", gd.ts),
                       p("view_off", gd.view_off), p("view_len", gd.view_len), p("seq", gd.seq))
    gp = b.gplan
    pl = codec._CommitOut(p("cm", gp.cm), p("topic_src", gp.topic_src), p("topic_kind", gp.topic_kind),
                          p("topic_off", gp.topic_off), p("topic_len", gp.topic_len), p("topic_idx", gp.topic_idx),
                          p("last", gp.last), p("count", gp.count))
    r = codec._CommitEmitOut(p("out_off", bufs["out_off"]), p("status", bufs["status"]), p("emit_idx", bufs["emit_idx"]),
                             p("totals", bufs["totals"]))
    rc = codec.lib().sbe_emit_commit_offsets(
        p("in", b.d), p("rec_off", b.ro), n, ctypes.byref(d), ctypes.byref(pl), p("topic_id", b.tid),
        p("ident_arena", b.itab[0]), p("ident_off", b.itab[1]), len(b.ids) if k is None else k, p("mask", mask),
        flags, session, 5, 6, p("out", bufs["out"]) if out else None, cap, ctypes.byref(r), p("ws", bufs["ws"]),
        bufs["ws"].numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module")
def small(codec):
    return Dev(codec, C.hand_records()[:13] + [_rec(i, i % 5 != 0) for i in range(300)], lead=1)


def test_contract_every_documented_element_and_nothing_else(codec, small):
    exp = small.expected(term=5, sess=6)
    m, total = int(exp["totals"][0]), int(exp["out_off"][-1])
    assert 0 < m < small.n

    def call(run):
        assert _raw(codec, small, run) == 0
        for key in ("out_off", "status", "totals"):
            run.expect(key, exp[key])
        run.expect("emit_idx", exp["emit_idx"])
        run.expect_poison("emit_idx", 8 * m)
        run.expect("out", exp["out"])
        run.expect_poison("out", total)

    G.twice(call)


def test_contract_repeated_call_is_identical(codec, small):
    runs = []
    for _ in range(2):
        run = G.PoisonRun(0x5A)
        assert _raw(codec, small, run) == 0
        run.check_guards()
        runs.append({k: run[k].numpy().copy() for k in ("out_off", "status", "emit_idx", "totals", "out")})
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k


EINVAL_CASES = {
    "k=0": dict(k=0), "k=65": dict(k=65), "unknown flag": dict(flags=2), "session=2": dict(session=2),
    "last_only with mask": dict(flags=C.LAST_ONLY, mask=True), "out null with capacity": dict(out=False),
    "null in": dict(null=("in",)), "null rec_off": dict(null=("rec_off",)), "null topic_id": dict(null=("topic_id",)),
    "null ident_off": dict(null=("ident_off",)), "null cm": dict(null=("cm",)), "null view_len": dict(null=("view_len",)),
    "null status": dict(null=("status",)), "null workspace": dict(null=("ws",)), "null totals": dict(null=("totals",)),
    "rec_off + 4": dict(shifts={"rec_off": 4}), "view_off + 2": dict(shifts={"view_off": 2}),
    "seq + 4": dict(shifts={"seq": 4}), "topic_idx + 2": dict(shifts={"topic_idx": 2}),
    "topic_id + 2": dict(shifts={"topic_id": 2}), "ident_off + 1": dict(shifts={"ident_off": 1}),
    "out_off + 4": dict(shifts={"out_off": 4}), "emit_idx + 4": dict(shifts={"emit_idx": 4}),
    "totals + 4": dict(shifts={"totals": 4}), "workspace + 8": dict(shifts={"ws": 8}),
}


@pytest.mark.parametrize("case", EINVAL_CASES, ids=list(EINVAL_CASES))
def test_contract_einval_writes_nothing(codec, small, case):
    kw = dict(EINVAL_CASES[case])
    if kw.get("mask") is True:
        kw["mask"] = torch.ones(small.n, dtype=torch.uint8, device="cuda")
    run = G.PoisonRun(0xA5)
    assert _raw(codec, small, run, **kw) == -1
    for name in run.bufs:
        run.expect_poison(name)
    run.check_guards()


def test_contract_empty_batch(codec, small):
    def call(run):
        assert _raw(codec, small, run, n=0, null=("in", "rec_off", "cm", "topic_id", "status", "ws")) == 0
        run.expect("out_off", [0])
        run.expect_poison("out_off", 8)
        run.expect("totals", [0, 0, 0])
        for name in ("status", "emit_idx", "out", "ws"):
            run.expect_poison(name)

    G.twice(call)
    r = codec.emit_commit_offsets(torch.zeros(0, dtype=torch.uint8, device="cuda"),
                                  torch.zeros(1, dtype=torch.int64, device="cuda"), small.gdec, small.gplan,
                                  small.tid, small.itab)
    torch.cuda.synchronize()
    assert r.numpy()["totals"].tolist() == [0, 0, 0] and r.status.numel() == 0
