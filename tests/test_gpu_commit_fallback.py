"""GPU: sbe_emit_commit_offsets_ex with a fallback: the legacy COMMIT_OFFSET TopicMessage of topics
without a numeric id beside the CommitOffsetLite frames, compacted on the device.  Every output
(out, out_off, status, emit_idx, totals) is compared byte for byte and element for element with
commitfallback_lib.ref_emit, a composition of the restated plan, commitsend_lib.ref_emit, a few
lines of text pinned to the oracle's quoting, and the oracle's TopicMessage encoder.  The decode
and classify outputs the call consumes are the device's own.  The quoting helper of the kernels
(oj::quoted) runs only here: the host build of the CPU suite cannot hold it."""
import ctypes

import numpy as np
import pytest
import torch

import autocommit_lib as A
import commitfallback_lib as F
import commitsend_lib as C
import contract_lib as G
import sbe_testlib as T
from test_commit_fallback_ref import _bound_batch, wrap_records
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu
SENTINEL = 0xEE
POISON_I64 = C.POISON - 2**64


class Dev:
    """A batch on the device: decoded (seq pre-filled with a poison) and classified there."""

    def __init__(self, codec, recs, lead=0, topics=F.TOPICS, ids=F.TOPIC_IDS, idents=F.IDENTS, default=F.DEFAULT_IDENT):
        self.codec, self.topics, self.ids, self.idents, self.default = codec, topics, ids, idents, default
        self.data, self.off, self.dec, self.seq = C.batch(recs, lead)
        self.n = self.off.size - 1
        self.plan = A.ref_classify(self.data, self.off, self.dec, topics)
        self.d = to_dev(self.data if self.data.size else np.zeros(16, np.uint8), torch.uint8)
        self.ro = to_dev(self.off.astype(np.uint64), torch.int64)
        seq = torch.full((max(self.n, 1),), POISON_I64, dtype=torch.int64, device="cuda")
        self.gdec = codec.decode_batch(self.d, self.ro, mode=codec.DEC_PARSE_MESSAGE, seq=seq)
        self.ttab = codec.commit_topic_table(topics, "cuda")
        self.gplan = codec.classify_commits(self.d, self.ro, self.gdec, self.ttab)
        self.tid = to_dev(np.asarray(ids, np.uint32), torch.int32)
        self.itab = codec.commit_identifier_table(idents, "cuda")
        self.dident = to_dev(np.frombuffer(default, np.uint8).copy() if default else np.zeros(0, np.uint8), torch.uint8)
        self.fb = codec.CommitFallback(self.ttab, self.dident, F.NOW, F.UUID0)

    def expected(self, use_seq=True, **kw):
        return F.ref_emit(self.data, self.off, self.dec, self.plan, self.topics, self.ids, self.idents, self.default,
                          seq=self.seq if use_seq else None, **kw)

    def run(self, use_seq=True, mask=None, flags=0, session=True, term=0, sess=0, cap=None, out_shift=0, fb=True):
        exp_total = int(self.expected(use_seq, mask=mask, flags=flags, session=session)["out_off"][-1])
        cap = exp_total if cap is None else cap
        raw = torch.full((cap + out_shift + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        dec = self.gdec
        if not use_seq:
            dec = self.codec.Decoded(dec.status, dec.flags, dec.hdr, dec.ts, dec.view_off, dec.view_len, None)
        m = None if mask is None else to_dev(np.asarray(mask, np.uint8), torch.uint8)
        r = self.codec.emit_commit_offsets(self.d, self.ro, dec, self.gplan, self.tid, self.itab, mask=m, flags=flags,
                                           session=session, leadership_term_id=term, cluster_session_id=sess,
                                           out=raw[out_shift:], out_capacity=cap, fallback=self.fb if fb else None)
        torch.cuda.synchronize()
        got = r.numpy()
        assert (raw[:out_shift].cpu().numpy() == SENTINEL).all()
        return got

    def check(self, what="", **kw):
        exp = self.expected(**{k: v for k, v in kw.items() if k != "out_shift"})
        got = self.run(**kw)
        F.same(got, exp, what)
        tail = got["out"][exp["out"].size:]
        assert (tail == SENTINEL).all(), (what, "bytes written past the last frame that fits", np.nonzero(tail != SENTINEL)[0][:5])
        return got, exp


def _rec(i, kind, idn=None):
    """kind: 'json' (a topic outside the table / an id-0 entry / the fallback topic, in turn),
    'lite' or 'none'."""
    mid = (b"id-%d" % i) if idn is None else bytes([97 + i % 26]) * idn
    if kind == "none":
        return T.tm_wire([b"orders", b"SUBSCRIBE", b"s%d" % i, C.P, b"{}"], i)
    if kind == "lite":
        hd = [b'{"topic":"alpha"}', b'{"topic":"beta"}', b'{"topic":"orders"}', b'{"topic":""}'][i % 4]
    else:
        hd = [b'{"topic":"user-%d"}' % i, b'{"topic":"gamma"}', b"{}"][i % 3]
    return T.tm_wire([b"orders", b"X", mid, C.PSEQ if i % 5 == 0 else C.P, hd], 1_000_000 + i)


@pytest.mark.parametrize("pattern", ["all_json", "none", "alternating", "last_tile"])
# 257 reaches a second 256-record sizing block, 513 a third, with tiles past the second in a block
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257, 513])
def test_small_shapes(codec, n, pattern):
    first_of_last = (n - 1) // 64 * 64
    kind = {"all_json": lambda i: "json", "none": lambda i: "none", "alternating": lambda i: "json" if i % 2 else "lite",
            "last_tile": lambda i: "json" if i >= first_of_last else "none"}[pattern]
    b = Dev(codec, [_rec(i, kind(i)) for i in range(n)])
    got, exp = b.check((n, pattern), term=3, sess=4)
    want_json = sum(1 for i in range(n) if kind(i) == "json")
    assert (got["status"] == F.EMITTED_JSON).sum() == want_json
    assert int(got["totals"][0]) == sum(1 for i in range(n) if kind(i) != "none") and int(got["totals"][2]) == 0


@pytest.mark.parametrize("lead", [0, 7])
@pytest.mark.parametrize("use_seq", [True, False])
def test_hand_table_one_record_per_rule(codec, lead, use_seq):
    b = Dev(codec, F.hand_records(), lead=lead)
    got, exp = b.check(("hand", lead), use_seq=use_seq, term=-1, sess=2**62)
    assert list(got["status"]) == list(F.hand_status())
    assert (b.gdec.seq.cpu().numpy().view(np.uint64) == C.POISON).any()
    f2 = F.frame(got, 2)
    assert (b'"sequence_number":123456789012,' if use_seq else b'"sequence_number":0,') in f2


@pytest.mark.parametrize("through", ["identifier", "id"])
def test_bound_1040_emits_1041_does_not(codec, through):
    recs, topics, ids, idents, _ = _bound_batch(through)
    b = Dev(codec, recs, topics=topics, ids=ids, idents=idents)
    got, exp = b.check(through)
    assert list(got["status"]) == [F.EMITTED_JSON, F.E100]
    assert [int(x) for x in np.diff(got["out_off"])] == [32 + 1040, 0]


def test_u16_wrap(codec):
    """A 65535-byte id of 0x01 bytes (a text of over 6 * 65535 bytes), and ids that bring the text to
    65535, 65536 (an empty payload) and 65537 bytes."""
    b = Dev(codec, wrap_records(), lead=3)
    got, exp = b.check("wrap", session=False)
    assert list(got["status"]) == [F.EMITTED_JSON, F.E100, F.EMITTED_JSON, F.EMITTED_JSON]
    assert F.frame(got, 2).endswith(b"\x00\x00\x02\x00{}")


def test_multi_pass_window(codec):
    """A tile of 64 frames of about 1 KiB each (over the LDS window several times), and one more."""
    sk = 63 + 32 + len(F.uuid(F.DEFAULT_IDENT, F.UUID0)) + F.skeleton_len(b"user-10", F.DEFAULT_IDENT, 0, 1_000_000)
    recs = [T.tm_wire([b"orders", b"X", bytes([97 + i % 26]) * (1072 - sk - i % 40), C.P, b'{"topic":"user-%d"}' % (10 + i)],
                      1_000_000 + i) for i in range(70)]
    b = Dev(codec, recs)
    got, exp = b.check("multipass", term=1, sess=2)
    sizes = np.diff(got["out_off"])
    assert (got["status"] == F.EMITTED_JSON).all() and sizes.min() >= 1000 and sizes.max() == 1072
    assert int(got["out_off"][64]) > 4 * 16384


@pytest.mark.parametrize("out_shift", [0, 5])
@pytest.mark.parametrize("lead", [0, 7])
def test_alignment_sweep(codec, lead, out_shift):
    """JSON frames of varying id length; every tile's bytes are 1 mod 16, so the output bases of the
    17 tiles take every residue mod 16."""
    recs, tiles = [], 17
    for t in range(tiles):
        tile_bytes = 0
        for r in range(64):
            i = 64 * t + r
            fixed = 32 + 63 + len(F.uuid(F.DEFAULT_IDENT, F.UUID0 + i)) + \
                F.skeleton_len(b"u%04d" % i, F.DEFAULT_IDENT, 0, 1_000_000 + i)
            idn = 1 + (i * 7 + t) % 48
            if r == 63:
                idn = 1 + (1 - tile_bytes - fixed - 1) % 16 + 16 * (t % 3)
            tile_bytes += fixed + idn
            recs.append(T.tm_wire([b"orders", b"X", bytes([97 + i % 26]) * idn, C.P, b'{"topic":"u%04d"}' % i], 1_000_000 + i))
    recs += [T.tm_wire([b"orders", b"X", b"tail-%d" % i, C.P, b'{"topic":"alpha"}'], i) for i in range(5)]
    b = Dev(codec, recs, lead=lead)
    got, exp = b.check(("sweep", lead, out_shift), term=1, sess=2, out_shift=out_shift)
    assert {int(exp["out_off"][64 * t]) % 16 for t in range(tiles)} == set(range(16))
    assert (got["status"][:64 * tiles] == F.EMITTED_JSON).all()


@pytest.fixture(scope="module")
def rnd(codec):
    return Dev(codec, F.random_records(), lead=5)


def test_random_batch(rnd):
    got, exp = rnd.check("random", term=0x0102030405060708, sess=-2)
    cnt = np.bincount(got["status"], minlength=7)
    assert all(cnt[s] >= 1 for s in (F.NONE, F.EMITTED, F.HOST, F.E109, F.EMITTED_JSON, F.E100)), cnt
    assert cnt[F.EMITTED_JSON] * 10 >= rnd.n, cnt
    gp = rnd.gplan.numpy()
    for key in ("cm", "topic_idx", "topic_kind", "topic_off", "topic_len"):
        assert np.array_equal(gp[key], rnd.plan[key]), key


def test_mask_and_last_only(codec, rnd):
    mask = (np.arange(rnd.n) % 3 != 1).astype(np.uint8)
    got, _ = rnd.check("mask", mask=mask, term=7, sess=7)
    assert (got["status"][mask == 0] == F.NONE).all()
    got, _ = rnd.check("last_only", flags=F.LAST_ONLY, term=7, sess=7)
    assert got["status"][int(rnd.plan["last"][0])] == F.EMITTED_JSON
    with pytest.raises(codec.SbeError, match="EINVAL"):
        rnd.run(flags=F.LAST_ONLY, mask=mask)


@pytest.mark.parametrize("which", ["minus1", "mid", "early", "zero"])
def test_capacity(codec, rnd, which):
    full = rnd.expected(term=1, sess=1)
    total = int(full["out_off"][-1])
    cap = {"minus1": total - 1, "mid": int(full["out_off"][rnd.n // 2]) + 5, "early": int(full["out_off"][70]) - 1,
           "zero": 0}[which]
    if which == "zero":  # out = NULL sizes the batch
        r = codec.emit_commit_offsets(rnd.d, rnd.ro, rnd.gdec, rnd.gplan, rnd.tid, rnd.itab, leadership_term_id=1,
                                      cluster_session_id=1, out=None, out_capacity=0, fallback=rnd.fb)
        torch.cuda.synchronize()
        got = r.numpy()
        assert got["out"] is None
        got["out"] = np.zeros(0, np.uint8)
        F.same(got, rnd.expected(term=1, sess=1, cap=0), which)
    else:
        got, exp = rnd.check(which, term=1, sess=1, cap=cap)
        assert (got["status"] == F.OVERFLOW).any() and ((got["status"] == F.EMITTED) | (got["status"] == F.EMITTED_JSON)).any()
    assert np.array_equal(got["out_off"], full["out_off"]) and np.array_equal(got["totals"], full["totals"])
    assert np.array_equal(got["emit_idx"], full["emit_idx"])


def test_default_capacity_is_the_bound(codec, rnd):
    r = codec.emit_commit_offsets(rnd.d, rnd.ro, rnd.gdec, rnd.gplan, rnd.tid, rnd.itab, fallback=rnd.fb)
    torch.cuda.synchronize()
    got = r.numpy()
    F.same(got, rnd.expected(), "bound")
    assert got["out"].size >= int(got["totals"][1]) and (got["status"] != F.OVERFLOW).all()


def test_without_fallback_equals_the_plain_entry_point(codec, rnd):
    """fb == NULL through the new entry point: every output equals sbe_emit_commit_offsets'."""
    exp = C.ref_emit(rnd.data, rnd.off, rnd.dec, rnd.plan, F.TOPIC_IDS, F.IDENTS, seq=rnd.seq, term=4, sess=5)
    runs = []
    for ex in (False, True):
        run = G.PoisonRun(0x3C)
        assert _raw(codec, rnd, run, ex=ex, fb=False, full=int(exp["out_off"][-1])) == 0
        run.check_guards()
        runs.append({k: run[k].numpy().copy() for k in ("out_off", "status", "emit_idx", "totals", "out")})
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    assert np.array_equal(runs[1]["status"][:rnd.n], exp["status"]) and int(runs[1]["totals"][2]) > 100


# ------------------------------------------------------------------------------------------
# the call contract (include/sbecodec.h), through the C ABI with every buffer the test's
# ------------------------------------------------------------------------------------------
def _raw(codec, b, run, n=None, cap=None, mask=None, flags=0, session=1, k=None, out=True, shifts=None, null=(),
         ex=True, fb=True, full=None, ident_len=None):
    """sbe_emit_commit_offsets_ex (ex=False: sbe_emit_commit_offsets) with outputs from `run` at their
    minimal alignment.  shifts: extra byte offsets on named pointers; null: pointers passed as NULL."""
    n = b.n if n is None else n
    shifts = shifts or {}
    full = int(b.expected()["out_off"][-1]) if full is None else full
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
    args = [p("in", b.d), p("rec_off", b.ro), n, ctypes.byref(d), ctypes.byref(pl), p("topic_id", b.tid),
            p("ident_arena", b.itab[0]), p("ident_off", b.itab[1]), len(b.ids) if k is None else k, p("mask", mask),
            flags, session, 4, 5, p("out", bufs["out"]) if out else None, cap, ctypes.byref(r), p("ws", bufs["ws"]),
            bufs["ws"].numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)]
    if not ex:
        rc = codec.lib().sbe_emit_commit_offsets(*args)
    else:
        f = codec._CommitFallback(p("fb_arena", b.ttab[0]), p("fb_off", b.ttab[1]), p("fb_ident", b.dident),
                                  b.dident.numel() if ident_len is None else ident_len, F.NOW, F.UUID0)
        rc = codec.lib().sbe_emit_commit_offsets_ex(*args, ctypes.byref(f) if fb else None)
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module")
def small(codec):
    return Dev(codec, F.hand_records()[:13] + [_rec(i, ["json", "lite", "none"][i % 3]) for i in range(300)], lead=1)


def test_contract_every_documented_element_and_nothing_else(codec, small):
    exp = small.expected(term=4, sess=5)
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
    "last_only with mask": dict(flags=F.LAST_ONLY, mask=True), "out null with capacity": dict(out=False),
    "null in": dict(null=("in",)), "null rec_off": dict(null=("rec_off",)), "null topic_id": dict(null=("topic_id",)),
    "null ident_off": dict(null=("ident_off",)), "null cm": dict(null=("cm",)), "null view_len": dict(null=("view_len",)),
    "null status": dict(null=("status",)), "null workspace": dict(null=("ws",)), "null totals": dict(null=("totals",)),
    "rec_off + 4": dict(shifts={"rec_off": 4}), "view_off + 2": dict(shifts={"view_off": 2}),
    "seq + 4": dict(shifts={"seq": 4}), "topic_idx + 2": dict(shifts={"topic_idx": 2}),
    "topic_id + 2": dict(shifts={"topic_id": 2}), "ident_off + 1": dict(shifts={"ident_off": 1}),
    "out_off + 4": dict(shifts={"out_off": 4}), "emit_idx + 4": dict(shifts={"emit_idx": 4}),
    "totals + 4": dict(shifts={"totals": 4}), "workspace + 8": dict(shifts={"ws": 8}),
    # the fallback's own
    "null fb arena": dict(null=("fb_arena",)), "null fb topic_off": dict(null=("fb_off",)),
    "null default_ident": dict(null=("fb_ident",)), "default_ident_len 4097": dict(ident_len=4097),
    "fb topic_off + 2": dict(shifts={"fb_off": 2}), "null ts": dict(null=("ts",)), "ts + 4": dict(shifts={"ts": 4}),
    "null topic_kind": dict(null=("topic_kind",)), "null plan topic_off": dict(null=("topic_off",)),
    "null plan topic_len": dict(null=("topic_len",)), "plan topic_off + 2": dict(shifts={"topic_off": 2}),
    "plan topic_len + 1": dict(shifts={"topic_len": 1}),
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
                                  small.tid, small.itab, fallback=small.fb)
    torch.cuda.synchronize()
    assert r.numpy()["totals"].tolist() == [0, 0, 0] and r.status.numel() == 0
