"""CPU: tests/bigbatch_lib.py, the helpers of test_gpu_second_trip.py and test_gpu_far_input.py.

The sizes those tests use lie past the thresholds that follow from the constants of the sources,
with a partial last trip; the pool assembly gives what the oracle gives on a whole batch; and the
numpy restatements used where a Python loop over a million records is too slow give what the
restatements they stand for give."""
import os
import subprocess

import numpy as np
import pytest
import torch

import bigbatch_lib as B
import contract_lib as C
import publish_lib as P
import report_lib as R
import sbe_testlib as T
import termappend_lib as TA
import termpoll_lib as TP
import termscan_lib as TS

SWEEPS = ("dr_list_scan", "inf_rehash / inf_reset_values")  # table capacities are powers of two


def test_every_size_lies_past_its_threshold_with_a_partial_last_trip():
    c = B.constants()
    assert C.frag_scan_block() == c["SBE_FS_PER"] * c["kFsThreads"]
    t = B.trips(c)
    assert len(t) == 12
    for name, (items, per_trip) in t.items():
        assert items > per_trip, f"{name}: {items} items fit the {per_trip} of one trip"
        if name in SWEEPS:  # a sweep of a table: its slots are a whole number of trips, at least two
            assert items % per_trip == 0
        else:
            assert items % per_trip != 0, f"{name}: the last trip over {items} items is a full one"
            assert items < 2 * per_trip or name == "lat_report_final", name
    # the smallest sizes that reach the second trip today: a test that needs more must say so here
    assert B.N == 2 ** 20 + 1025 and B.N_COMMIT == 2 ** 19 + 257 and B.N_LAT == 2_097_152 + 4097
    assert B.LAT_CAPACITY == 2 ** 22 and (B.INF_BIG, B.INF_SMALL) == (2 ** 20, 2 ** 19)


def test_the_thresholds_of_the_table():
    """Where the second trip of every loop starts at today's constants."""
    c = B.constants()
    fs = c["SBE_FS_PER"] * c["kFsThreads"]
    assert fs * fs == 2 ** 20                                        # frag_scan_blocks: n > 2^20
    assert c["SBE_FC_MAXB"] * 4 * c["kFragGroup"] == 2 ** 20         # frag_copy: m + 1 > 2^20
    assert c["kMatBlk"] ** 2 == 2 ** 20                              # mat_scan_blocks; ta: n + 1 > 2^20
    assert 4 * c["kScanThreads"] * c["kBlock"] == 2 ** 20            # order_json_scan_blocks
    assert (4 * c["kScanThreads"] // 2 - 1) * c["kBlock"] == 524_032  # commit: 2 (nblk + 1) > 4096
    assert c["kDrSortBlocks"] * c["kDrBlk"] * c["kDrPer"] == 2_097_152 and c["kDrSortBlocks"] * c["kDrBlk"] == 262_144
    assert c["kDrListBlocks"] * c["kDrBlk"] == 2 ** 18 and c["kInfRehashBlocks"] * c["kInfBlk"] == 2 ** 19


# ------------------------------------------------------------------------------------------
# the pool method against the oracle on a whole batch
# ------------------------------------------------------------------------------------------
def test_assemble_is_a_gather():
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 9, 50)
    lens[:3] = 0
    off = B.rows_offsets(lens)
    pool = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    pick = rng.integers(0, 50, 1000)
    for chunk in (7, 1 << 18):
        got, got_off = B.assemble(torch.from_numpy(pool), torch.from_numpy(off), torch.from_numpy(pick), chunk=chunk)
        want = b"".join(pool[off[p]:off[p + 1]].tobytes() for p in pick)
        assert got.numpy().tobytes() == want
        assert got_off.tolist() == [0] + list(np.cumsum(lens[pick]))
    empty, e_off = B.assemble(torch.from_numpy(pool), torch.from_numpy(off), torch.from_numpy(np.array([0, 1, 2])))
    assert empty.numel() == 0 and e_off.tolist() == [0, 0, 0, 0]


def test_materialize_by_pool_matches_the_oracle_on_the_batch():
    data, off, dec = B.small_record_pool()
    assert off.size - 1 <= B.POOL and set(dec["status"].tolist()) == {T.ST_LITE, T.ST_TM}
    pool_arena, pool_arena_off = B.materialize_pool(data, off, dec)
    n = 10_007
    pk = B.Picked(torch.from_numpy(B.draw(n, off.size - 1, 3)))
    d, o = pk.ranges(data, off)
    arena, arena_off = B.materialize_expected(B.as_tensor(pool_arena), B.as_tensor(pool_arena_off),
                                              B.as_tensor(dec["view_len"]), pk.pick)
    # the oracle decodes and materializes the assembled batch itself, each kind in its mode
    d, o = d.numpy(), o.numpy().view(np.uint64)
    lite, tm = T.oracle_decode(d, o, T.DEC_LITE), T.oracle_decode(d, o, T.DEC_PARSE)
    is_lite = lite["status"] == T.ST_LITE
    whole = {k: np.where(is_lite.reshape((-1,) + (1,) * (lite[k].ndim - 1)), lite[k], tm[k]) for k in lite}
    for k in whole:
        assert np.array_equal(whole[k], dec[k][pk.pick.numpy()]), k
    want, want_off = T.oracle_materialize(d, o, whole)
    assert np.array_equal(want, arena.numpy()) and np.array_equal(want_off, arena_off.numpy().view(np.uint64))


@pytest.mark.parametrize("what", [0, 1])
def test_order_json_by_pool_matches_the_oracle_on_the_batch(what):
    b = P.mixed_batch(300, 5)
    arena, str_len = T.pack_order_fields(b.fields)
    text, text_off = T.oracle_order_json(arena, str_len, b.cid, b.ts, b.q, what)
    pk = B.Picked(torch.from_numpy(B.draw(10_000, b.n, 4)))
    got, got_off = pk.ranges(text, text_off)
    a, _ = pk.ranges(arena, B.rows_offsets(str_len.sum(1)))
    p = pk.pick.numpy()
    want, want_off = T.oracle_order_json(a.numpy(), str_len[p], b.cid[p], b.ts[p], b.q[p], what, nthreads=4)
    assert got.numpy().tobytes() == want and np.array_equal(got_off.numpy().view(np.uint64), want_off)
    assert np.array_equal(pk.rows(b.q).numpy().view(np.uint64), b.q[p].view(np.uint64))  # NaN payloads and -0.0 kept


def test_reassembly_arrays_match_the_list_form():
    data, frag_off, flags = T.fragment_stream(5000, 9, maxlen=8)
    msgs, carry = T.oracle_reassemble(data, frag_off, flags)
    out, msg_off, counts = B.oracle_reassemble_arrays(data, frag_off, flags)
    exp = C.reassembled_expected(msgs, carry)
    assert np.array_equal(out, exp[0]) and np.array_equal(msg_off, exp[1]) and np.array_equal(counts, exp[2])


def test_reassembly_streams_hold_their_properties():
    blk = C.frag_scan_block()
    data, frag_off, flags = B.frag_stream_singles()
    assert flags.size == B.N and int(frag_off[-1]) == data.size and np.diff(frag_off.astype(np.int64)).max() == 8
    _, msg_off, counts = B.oracle_reassemble_arrays(data, frag_off, flags)
    assert int(counts[0]) >= 2 ** 20 + 1 and 0 < (flags != B.SINGLE).sum() < 1024
    for name, (data, frag_off, flags, k) in B.frag_streams_structured(blk).items():
        assert flags.size == B.N_FRAG_B and k["b"] < blk * blk, name
        _, _, counts = B.oracle_reassemble_arrays(data, frag_off, flags)
        assert name != "carry" or int(counts[1]) > 1000  # the random tails of the others may leave a few bytes open


# ------------------------------------------------------------------------------------------
# the numpy restatements
# ------------------------------------------------------------------------------------------
def test_term_append_np_matches_the_python_loop():
    for long_at, limit, spare in (((), None, 96), ((700,), None, 96), ((300, 700), None, 96), ((), 40_000, 96),
                                  ((), None, -4000), ((), None, -31 * 32), ((500,), 20_000, 96)):
        data, rec_off = B.term_append_records(1000, long_at, seed=len(long_at))
        frames = sum(TA.required(int(x), 1408) for x in np.diff(rec_off.astype(np.int64)) if x <= B.TA_MAX_LEN)
        nb = 64 + frames + spare
        nb -= nb % 32
        want = TA.append_offsets(TA.sentinel(nb), 64, data.tobytes(), [int(x) for x in rec_off], limit=limit,
                                 max_message_length=B.TA_MAX_LEN)
        got = B.term_append_np(nb, 64, data, rec_off, limit=limit)
        assert got["block"].tobytes() == want["block"], (long_at, limit, spare)
        assert [got[k] for k in ("appended", "next", "payload", "stop")] == [want[k] for k in ("appended", "next", "payload", "stop")]
        assert got["rec_tail"].tolist() == want["rec_tail"]
    stops = {B.term_append_np(64 + 4000, 64, *B.term_append_records(1000, ()), limit=lim)["stop"] for lim in (None, 1000)}
    assert stops == {TA.TRIPPED, TA.LIMIT}


def test_term_append_np_matches_the_host_mirror_at_full_size(tmp_path):
    """The three runs of the GPU test, on the same arrays, through the stand-alone program over the
    host mirror's serial term_append (tests/termappend/term_append_main.cpp)."""
    path = tmp_path / "big_cases.bin"
    runs = B.term_append_runs(B.constants()["kMatBlk"])
    with open(path, "wb") as f:
        f.write(np.uint64(len(runs)).tobytes())
        for name, data, rec_off, block_bytes, stop, long_at in runs:
            exp = B.term_append_np(block_bytes, 64, data, rec_off)
            assert exp["stop"] == stop and exp["appended"] == (min(long_at) if long_at else B.N), name
            B.write_term_append_case(f, block_bytes, 64, data, rec_off, exp)
    subprocess.run(["make", "-s", "-C", TA.DIR, "term_append_check"], check=True)
    r = subprocess.run([os.path.join(TA.DIR, "term_append_check"), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "term append: %d cases ok" % len(runs) in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_term_poll_block_matches_the_walk_and_the_composition():
    """The table known by construction is termscan_lib.walk's, and the arrays are
    termpoll_lib.expect's, with and without a carry."""
    block, payload, frag_off, flags = B.term_poll_block(10_000, edge=5000, seed=3)
    w = TS.walk(block.tobytes())
    assert (w["fragments"], w["next"], w["stop"]) == (10_000, block.size, TS.END)
    assert w["flags"] == flags.tolist() and w["frag_off"] == frag_off.tolist() and w["payload"] == payload.tobytes()
    assert set(np.diff(np.array(w["frag_src"] + [block.size]))) == {32, 64}
    assert {B.BEGIN, B.END, B.MIDDLE, B.SINGLE} == set(flags.tolist())
    assert flags[4998:5002].tolist() == [B.BEGIN, B.MIDDLE, B.MIDDLE, B.END]
    for carry in (b"", TP.carry_bytes(1000)):
        want = TP.expect(block.tobytes(), carry=carry)
        got = B.term_poll_expected(block.size, payload, frag_off, flags, carry)
        assert got["counts"] == want["counts"]
        assert got["out"].tobytes() == b"".join(want["msgs"]) + want["carry"]
        assert got["msg_off"].tolist() == [0] + list(np.cumsum([len(m) for m in want["msgs"]]))


def test_inflight_key_helpers():
    keys = B.hex_keys(5000, 1)
    ks = B.key_list(keys)
    assert len(set(ks)) == 5000 and all(len(k) == 16 and k[:1] == b"k" for k in ks)
    data, off = B.ack_records(keys[:100], 777)
    import inflight_lib as I
    assert data.tobytes() == b"".join(I.full_ack(k, b"orders", b"c", 777) for k in ks[:100])
    exp = T.oracle_decode(data, off, T.DEC_EGRESS)
    assert [a[1] for a in I.acks_of(data, off, exp)] == ks[:100]
    # table_entries reads a slot as csrc/inflight.hpp lays it out: word, value, five key words, claim | len << 32
    words = np.zeros((8, 8), np.uint64)
    words[3] = [(2 << 62) | 1, 99] + list(np.frombuffer(ks[0] + bytes(24), "<u8")) + [16 << 32]
    words[5] = [3 << 62, 7] + list(np.frombuffer(ks[1] + bytes(24), "<u8")) + [16 << 32]  # erased
    slots, got, values, answered = B.table_entries(words)
    assert slots.tolist() == [3] and got.tolist() == [ks[0]] and values.tolist() == [99] and answered.tolist() == [True]


def test_report_np_matches_report_lib():
    rng = np.random.default_rng(7)
    for n in (0, 1, 2, 1000, 5001):
        lats = rng.integers(-50, 50, n) if n != 1000 else rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64, endpoint=True)
        want, got = R.report([int(v) for v in lats]), B.report_np(lats)
        assert got["count"] == want["count"]
        for k in ("stats", "pct_value", "pct_index", "sorted", "order"):
            assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, (n, k)
