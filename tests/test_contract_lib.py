"""CPU test of the guard / poison bookkeeping of contract_lib.py on CPU tensors: a planted stray
write in a guard band and a planted unwritten element are both reported, and a clean run is not."""
import numpy as np
import pytest
import torch

import contract_lib as C


def test_view_sits_between_poisoned_bands():
    g = C.guarded(40, torch.int64, 8, 0x5A, device="cpu")
    assert g.t.numel() == 5 and g.t.dtype == torch.int64 and g.lo == C.GUARD + 8
    assert g.raw.numel() == C.GUARD + 8 + 40 + C.GUARD
    assert g.t.data_ptr() - g.raw.data_ptr() == C.GUARD + 8
    assert (g.numpy() == 0x5A5A5A5A5A5A5A5A).all() and g.untouched()
    g.check_guards()
    g.t.fill_(7)  # writing the view itself is no stray write
    g.check_guards()
    assert not g.untouched() and g.untouched(40, 40)


@pytest.mark.parametrize("where", [-1, -C.GUARD - 8, 40, 40 + C.GUARD - 1])
def test_stray_write_in_a_band_is_reported(where):
    g = C.guarded(40, torch.int64, 8, 0xA5, device="cpu", name="out_off")
    g.raw[g.lo + where] = 0
    assert g.stray_writes().tolist() == [where]
    with pytest.raises(AssertionError, match="out_off: 1 bytes written outside"):
        g.check_guards()


def test_stray_write_of_the_other_poison_is_reported():
    g = C.guarded(16, torch.uint8, 1, C.POISONS[0], device="cpu")
    g.raw[g.lo + 16] = C.POISONS[1]
    with pytest.raises(AssertionError):
        g.check_guards()


def test_unwritten_element_is_reported_whatever_the_oracle_value():
    """The oracle value of the skipped element equals one poison: that run alone would pass, the
    pair does not."""
    exp = np.array([3, 0x5A5A5A5A5A5A5A5A, 0, 9], np.uint64)

    def call(run, skip):
        t = run.buf("seq", 4, torch.int64, align=8)
        for i in range(4):
            if i != skip:
                t[i] = int(exp[i])
        run.expect("seq", exp)

    C.twice(lambda run: call(run, None), device="cpu")  # every element written: clean
    with pytest.raises(AssertionError, match=r"1 of them still hold the poison 0xA5 \(never written\)"):
        C.twice(lambda run: call(run, 1), device="cpu")  # passes under 0x5A, caught under 0xA5
    with pytest.raises(AssertionError, match=r"1 of them still hold the poison 0x5A \(never written\)"):
        C.twice(lambda run: call(run, 2), device="cpu")


def test_twice_checks_the_guards_of_every_buffer():
    def call(run):
        a = run.buf("status", 5, torch.uint8)
        run.buf("out", 32, torch.uint8, align=16)
        a.fill_(1)
        run["out"].bytes.fill_(2)
        run["out"].raw[run["out"].lo + 32] = 2  # one byte past the array
        run.expect("status", np.ones(5, np.uint8))

    with pytest.raises(AssertionError, match="out: 1 bytes written outside the array, at offsets \\[32\\]"):
        C.twice(call, device="cpu")


def test_expect_poison_and_mismatch_message():
    run = C.PoisonRun(0x5A, device="cpu")
    t = run.buf("seq", 6, torch.int64)
    t[2] = 11
    run.expect_poison("seq", 0, 16)
    run.expect_poison("seq", 24)
    with pytest.raises(AssertionError, match="seq: 8 bytes written where nothing may be, first at byte \\[16 17"):
        run.expect_poison("seq")
    assert C.mismatches(np.array([1, 2]), np.array([1, 2]), 0x5A) is None
    msg = C.mismatches(np.array([1, 0x5A, 7], np.uint8), np.array([1, 2, 3], np.uint8), 0x5A, "status")
    assert "status: 2 of 3 elements differ" in msg and "1 of them still hold the poison 0x5A" in msg


def test_expect_head_reports_a_write_behind_the_table():
    """A table of device-decided length: entries 0..k hold the values, the rest the poison."""
    def call(run, stray):
        t = run.buf("frag_off", 6, torch.int64)
        t[:3] = torch.tensor([0, 5, 9])
        if stray is not None:
            t[stray] = 9
        run.expect_head("frag_off", [0, 5, 9])

    C.twice(lambda run: call(run, None), device="cpu")
    with pytest.raises(AssertionError, match="frag_off: 8 bytes written where nothing may be, first at byte \\[40"):
        C.twice(lambda run: call(run, 5), device="cpu")
    with pytest.raises(AssertionError, match="frag_off: 1 of 3 elements differ"):
        C.twice(lambda run: call(run, 1), device="cpu")


def test_expect_rows_reports_writes_outside_the_slice():
    def call(run, stray):
        t = run.buf("view_off", 5 * 6, torch.int32)
        t[5 * 2: 5 * 4] = torch.arange(10, dtype=torch.int32)
        if stray is not None:
            t[stray] = 1
        run.expect_rows("view_off", np.arange(10), 2, per=5)

    C.twice(lambda run: call(run, None), device="cpu")
    for stray, first in ((9, 36), (20, 80), (29, 116)):  # the row in front, the row behind, the last element
        with pytest.raises(AssertionError, match="view_off: 4 bytes written where nothing may be, first at byte \\[%d" % first):
            C.twice(lambda run: call(run, stray), device="cpu")


def test_workspace_history_order_and_fills():
    ws = torch.full((8,), 0x5A, dtype=torch.uint8)
    seen = []
    C.workspace_history(ws, lambda w: (seen.append(("big", int(w[0]))), w.fill_(1)),
                        lambda w: (seen.append(("small", int(w[0]))), w.fill_(2)), fills=(0xFF, 0x00, 0x80))
    assert seen == [("big", 0x5A), ("small", 1), ("small", 0xFF), ("big", 0xFF), ("small", 0), ("big", 0),
                    ("small", 0x80), ("big", 0x80)]


def test_minimal_alignment_and_placed_inputs():
    assert C.min_shift(torch.int64) == 8 and C.min_shift(torch.uint8) == 1 and C.min_shift(torch.uint8, 16) == 16
    off = np.arange(7, dtype=np.uint64) * 3
    t = C.placed(off, 8, device="cpu")
    assert t.dtype == torch.int64 and t.tolist() == list(range(0, 21, 3))
    L = np.arange(10, dtype=np.uint32).reshape(2, 5)
    assert C.placed(L, 4, device="cpu").shape == (2, 5)


def test_frag_scan_block_is_read_from_the_kernel_source():
    assert C.frag_scan_block() == 1024


def test_reassembled_expected():
    data, off, counts = C.reassembled_expected([b"ab", b"", b"cde"], b"xy")
    assert data.tobytes() == b"abcdexy" and off.tolist() == [0, 2, 2, 5] and counts.tolist() == [3, 2]
