"""CPU: the sequential model of ack correlation (tests/inflight_lib.py) on a hand table, and the
properties of the generated sequence the GPU test relies on."""
import numpy as np

import inflight_lib as I
import sbe_testlib as T

ACK, SIMPLE, TM = T.ST_EG_ACK, T.ST_EG_ACK_SIMPLE, T.ST_EG_TM
SEED = 4  # of the random sequence of tests/test_gpu_inflight.py


def test_duplicate_remember_keeps_the_first_ts():
    m = I.Model()
    st = m.remember([b"k1", b"k2", b"k1"], np.array([10, 20, 30], np.uint64))
    assert list(st) == [I.INF_INSERTED, I.INF_INSERTED, I.INF_DUPLICATE]
    assert list(m.remember([b"k2"], np.array([99], np.uint64))) == [I.INF_DUPLICATE]
    assert m.inflight == {b"k1": 10, b"k2": 20} and (m.live, m.used) == (2, 2)


def test_second_ack_of_one_id_is_unmatched():
    m = I.Model()
    m.remember([b"k1"], np.array([10], np.uint64))
    code, base, counts = m.match([(ACK, b"k1", 500), (ACK, b"k1", 600), (ACK, b"other", 700)])
    assert list(code) == [I.ACK_MATCHED, I.ACK_UNMATCHED, I.ACK_UNMATCHED]
    assert list(base) == [10, 600, 700] and list(counts) == [1, 2]
    assert (m.live, m.used) == (0, 1)


def test_simple_acks_and_empty_ids_never_match():
    m = I.Model()
    assert list(m.remember([b""], np.array([10], np.uint64))) == [I.INF_INSERTED]  # emplace("") succeeds
    code, base, counts = m.match([(SIMPLE, b"", 500), (ACK, b"", 600), (TM, b"", 700), (T.ST_EG_NONE, b"", 1)])
    assert list(code) == [I.ACK_UNMATCHED, I.ACK_UNMATCHED, I.ACK_NONE, I.ACK_NONE]
    assert list(base) == [500, 600, 0, 0] and list(counts) == [0, 2]
    assert m.live == 1


def test_remember_after_a_match_reinserts():
    m = I.Model()
    m.remember([b"k1"], np.array([10], np.uint64))
    m.match([(ACK, b"k1", 500)])
    assert list(m.remember([b"k1"], np.array([0], np.uint64), ts_default=77)) == [I.INF_INSERTED]
    assert m.inflight == {b"k1": 77} and (m.live, m.used) == (1, 2)
    code, base, _ = m.match([(ACK, b"k1", 900)])
    assert list(code) == [I.ACK_MATCHED] and list(base) == [77]


def test_mask_ts_rules_and_long_keys():
    m = I.Model()
    long = b"z" * 41
    st = m.remember([b"a", b"b", long, b"c"], np.array([0, 5, 6, 7], np.uint64), ts_default=42,
                    mask=np.array([1, 0, 1, 1], np.uint8))
    assert list(st) == [I.INF_INSERTED, I.INF_SKIPPED, I.INF_KEY_TOO_LONG, I.INF_INSERTED]
    assert m.inflight == {b"a": 42, b"c": 7}
    assert list(m.remember([b"d"], None, ts_default=9)) == [I.INF_INSERTED] and m.inflight[b"d"] == 9
    code, base, counts = m.match([(ACK, long, 300)])
    assert list(code) == [I.ACK_LONG_ID] and list(base) == [300] and list(counts) == [0, 1]
    ref = I.Model(key_max=None)  # the reference itself has no key limit
    assert list(ref.remember([long], np.array([6], np.uint64))) == [I.INF_INSERTED]
    assert list(ref.match([(ACK, long, 300)])[0]) == [I.ACK_MATCHED]


def test_padding_and_length_make_distinct_keys():
    m = I.Model()
    keys = [b"a", b"a\0", b"a\0\0", b"b", b"x" * 39 + b"y", b"x" * 40, b"x" * 39]
    assert list(m.remember(keys, np.arange(1, 8, dtype=np.uint64))) == [I.INF_INSERTED] * 7
    code, base, _ = m.match([(ACK, k, 0) for k in reversed(keys)])
    assert list(code) == [I.ACK_MATCHED] * 7 and list(base) == [7, 6, 5, 4, 3, 2, 1]


def test_random_sequence_holds_every_class():
    """The generated sequence of the GPU test, run through the model and the oracle alone."""
    pool, ops = I.random_ops(SEED)
    assert len(pool) == len(set(pool)) == 400 and {len(k) for k in pool} >= set(I.EDGE_LENS)
    m = I.Model()
    st_seen, code_seen, dec_seen = set(), set(), set()
    for op in ops:
        if op[0] == "remember":
            assert len(op[1]) <= 300
            st_seen |= set(m.remember(op[1], op[2], 5, op[3]))
        else:
            assert len(op[1]) <= 300
            data, off = T.pack_records(op[1])
            dec = T.oracle_decode(data, off, T.DEC_EGRESS)
            dec_seen |= set(dec["status"])
            acks = I.acks_of(data, off, dec)
            assert any(st == T.ST_EG_ACK and not mid for st, mid, _ in acks)
            code_seen |= set(m.match(acks)[0])
        assert m.used < 2048
    assert len(ops) == 20
    assert all(v >= 20 for v in m.seen.values()), m.seen
    assert st_seen == {I.INF_INSERTED, I.INF_DUPLICATE, I.INF_SKIPPED, I.INF_KEY_TOO_LONG}
    assert code_seen == {I.ACK_NONE, I.ACK_MATCHED, I.ACK_UNMATCHED, I.ACK_LONG_ID}
    assert dec_seen >= {T.ST_EG_ACK, T.ST_EG_ACK_SIMPLE, T.ST_EG_TM} and len(dec_seen) > 3  # and undecodable ones
