"""GPU: sbe_order_select against the sequential model of tests/select_lib.py.  Every comparison is
exact.  The edge batch (tests/test_select_lib.py checks what it holds) is decoded on the device
first; the call contract is checked as tests/test_gpu_contract.py checks the other entry points'."""
import numpy as np
import pytest
import torch

import contract_lib as C
import select_lib as S
import sbe_testlib as T
from test_gpu_contract import side_stream

pytestmark = pytest.mark.gpu

U8, I64 = torch.uint8, torch.int64
DEC_KEYS = ("status", "flags", "hdr", "ts", "view_off", "view_len")
OUT = ("pred", "select", "topic_class")


def dev(a):
    a = np.array(a, order="C")
    if a.dtype.kind in "ui":
        a = a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(a).cuda()


@pytest.fixture(scope="module")
def edge(codec):
    W = codec.order_select_window()
    assert W == S.window()
    names, data, off, dec = S.edge_case(W)
    exp = S.model(data, off, dec)
    S.check_composition(names, data, off, dec, exp, W)
    d, ro = dev(data), dev(off)
    assert d.data_ptr() % 16 == 0
    ddec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE)
    got = ddec.numpy()
    for k in DEC_KEYS:  # the device's own descriptors are the oracle's
        assert np.array_equal(got[k], dec[k]), k
    return names, data, off, dec, exp, d, ro, ddec


def dec_placed(codec, dec):
    """The descriptors at their minimal alignment (hdr 2 B, views 4 B); ts is not read."""
    return codec.Decoded(C.placed(dec["status"], 1), C.placed(dec["flags"], 1), C.placed(dec["hdr"], 2),
                         C.placed(dec["ts"], 8), C.placed(dec["view_off"], 4), C.placed(dec["view_len"], 4))


def test_edge_batch(codec, edge):
    names, data, off, dec, exp, d, ro, ddec = edge
    got = codec.order_select(d, ro, ddec)
    first = got.numpy()
    S.same(first, exp, "edge batch", names)
    again = codec.order_select(d, ro, ddec, out=got).numpy()  # the same arrays: totals are zeroed by the call
    S.same(again, exp, "repeated call", names)


@pytest.mark.parametrize("shift", [1, 6, 15])
def test_edge_batch_at_other_alignments(codec, edge, shift):
    names, data, off, dec, exp, d, ro, ddec = edge
    S.same(codec.order_select(C.placed(data, shift), ro, ddec).numpy(), exp, f"shift {shift}", names)


def test_non_default_stream(codec, edge):
    names, data, off, dec, exp, d, ro, ddec = edge
    # the suite's one side stream: a stream made here would move the streams made after it, the
    # serve tests' among them, onto other hardware queues
    s = side_stream(torch.empty(1 << 26, dtype=U8, device="cuda"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = codec.order_select(d, ro, ddec, stream=s)
    s.synchronize()
    S.same(got.numpy(), exp, "stream", names)


def test_writes_its_outputs_only(codec, edge):
    names, data, off, dec, exp, d, ro, ddec = edge
    n, extra = len(names), 9
    ro_p, dec_p = C.placed(off, 8), dec_placed(codec, dec)

    def one(run):
        out = codec.MessageKinds(*(run.buf(k, n + extra, U8) for k in OUT), run.buf("totals", 2, I64, 8))
        codec.order_select(d, ro_p, dec_p, out=out)
        torch.cuda.synchronize()
        for k in OUT + ("totals",):
            run.expect(k, exp[k])
        for k in OUT:
            run.expect_poison(k, n, n + extra)
        assert np.array_equal(d.cpu().numpy(), data)
    C.twice(one)


@pytest.mark.parametrize("absent", ["select", "topic_class"])
def test_null_outputs(codec, edge, absent):
    names, data, off, dec, exp, d, ro, ddec = edge
    got = codec.order_select(d, ro, ddec, want_select=absent != "select", want_class=absent != "topic_class")
    assert getattr(got, absent) is None
    S.same(got.numpy(), exp, f"no {absent}", names, keys=tuple(k for k in OUT + ("totals",) if k != absent))


def test_empty_batch(codec, edge):
    d = edge[5]

    def one(run):
        out = codec.MessageKinds(*(run.buf(k, 4, U8) for k in OUT), run.buf("totals", 2, I64, 8))
        codec.order_select(d, dev(np.zeros(1, np.uint64)), codec.alloc_decoded(0, "cuda"), out=out)
        torch.cuda.synchronize()
        run.expect("totals", [0, 0])
        for k in OUT:
            run.expect_poison(k)
    C.twice(one)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches(codec, edge, n):
    """Whole and partial tiles: the first n records of the search tile of the edge batch."""
    names, data, off, dec, exp, d, ro, ddec = edge
    a = names.index("lane0_needle")
    sub = {k: v[a:a + n] for k, v in dec.items()}
    e = S.model(data, off[a:a + n + 1], sub)
    got = codec.order_select(d, dev(off[a:a + n + 1]), codec.Decoded(*(dev(sub[k]) for k in DEC_KEYS))).numpy()
    S.same(got, e, f"n={n}", names[a:a + n])
    assert e["select"][0] == 1 and (n < 64 or e["select"][63] == 1)


def test_mutated_records(codec):
    data, off, dec = S.mutated_case(3000, 0x5E1)
    exp = S.model(data, off, dec)
    d, ro = dev(data), dev(off)
    ddec = codec.decode_batch(d, ro, mode=codec.DEC_PARSE_MESSAGE)
    S.same(codec.order_select(d, ro, ddec).numpy(), exp, "mutated")


def test_descriptor_clamping(codec, edge):
    """Views edited after the decode to point past their records: the result is the model's over the
    clamped views, and needles behind the last record decide nothing."""
    names, data, off, dec, _, _, _, _ = edge
    keep = [i for i in range(len(names)) if off[i + 1] - off[i] < 1024]
    recs = [bytes(data[int(off[i]):int(off[i + 1])]) for i in keep] + [S.tm(payload=b"xx"), S.tm(mtype=b"xx", payload=b"{}")]
    d2, o2 = T.pack_records(recs)
    dec2 = T.oracle_decode(d2, o2, T.DEC_PARSE)
    n = len(recs)
    rng = np.random.default_rng(11)
    for i in range(0, n - 2, 3):
        k = rng.integers(0, 5)
        dec2["view_len"][i, k] = (int(dec2["view_len"][i, k]) + int(rng.choice([1, 16, 40, 2 ** 31, 2 ** 32 - 1]))) & 0xFFFFFFFF
    for i in range(1, n - 2, 3):
        dec2["view_off"][i, rng.integers(0, 5)] = rng.choice([0, 20, 300, 2 ** 32 - 1])
    dec2["view_len"][n - 2, 3] = 4000       # the payload of the last but one runs on into the last record's type ...
    dec2["view_len"][n - 1, 1] = 100        # ... whose type and payload run on behind the batch
    dec2["view_len"][n - 1, 3] = 2 ** 32 - 1
    behind = b' ORDER TopicMessage side quantity client_order_id order_details token_pair ' * 4
    whole = np.concatenate([d2, np.frombuffer(behind, np.uint8)])
    exp = S.model(d2, o2, dec2)
    assert exp["select"][n - 1] == 0 and exp["select"][n - 2] == 0 and exp["pred"][n - 1] == S.PR_TOPIC_MESSAGE
    unclamped = bytes(whole[int(o2[n - 1]) + int(dec2["view_off"][n - 1, 3]):])
    assert b"side" in unclamped and (exp["select"] != S.model(d2, o2, T.oracle_decode(d2, o2, T.DEC_PARSE))["select"]).sum() >= 5
    got = codec.order_select(dev(whole), dev(o2), codec.Decoded(*(dev(dec2[k]) for k in DEC_KEYS))).numpy()
    S.same(got, exp, "clamped views", [names[i] for i in keep] + ["tail_payload", "tail_type"])
