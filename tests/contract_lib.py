"""Helpers of test_gpu_contract.py: the call contract of the batch entry points (include/sbecodec.h).

Outputs and workspaces are handed to the kernels as views into larger allocations: at the minimal
alignment the header promises, between two guard bands, and filled with a poison byte.  A call is
run twice, once per poison; every documented output must equal the oracle both times.  An element
a kernel never writes holds the poison both times, and no oracle value equals both poisons, so it
is reported whatever the right answer is; a byte written outside the documented arrays lands in a
guard band.  The bookkeeping is plain tensor arithmetic and works on CPU tensors
(tests/test_contract_lib.py)."""
import ctypes
import os
import re

import numpy as np
import torch

POISONS = (0x5A, 0xA5)
GUARD = 256

_NP = {torch.uint8: np.uint8, torch.int16: np.uint16, torch.int32: np.uint32, torch.int64: np.uint64}


def poison_value(poison: int, np_dtype):
    """The element an array of np_dtype holds where it was never written."""
    return np.frombuffer(bytes([poison]) * np.dtype(np_dtype).itemsize, np_dtype)[0]


class Guarded:
    """`nbytes` at base + GUARD + shift of one allocation, as a tensor of `dtype` (self.t), filled
    with `poison`, with GUARD poison bytes before it and at least GUARD after it."""

    def __init__(self, nbytes, dtype, shift, poison, device="cuda", name="buffer"):
        item = torch.empty(0, dtype=dtype).element_size()
        assert nbytes % item == 0 and shift % item == 0 and 0 <= shift < GUARD, (nbytes, item, shift)
        self.name, self.nbytes, self.lo, self.poison = name, int(nbytes), GUARD + shift, poison
        self.raw = torch.full((GUARD + shift + self.nbytes + GUARD,), poison, dtype=torch.uint8, device=device)
        if self.raw.is_cuda:  # the alignment of the view is exactly `shift` past a 256-byte boundary
            assert self.raw.data_ptr() % GUARD == 0
        self.bytes = self.raw[self.lo: self.lo + self.nbytes]
        self.t = self.bytes.view(dtype)

    def fill(self, poison):
        self.raw.fill_(poison)
        self.poison = poison

    def stray_writes(self):
        """Offsets, relative to the view's first byte, of guard bytes that lost the poison."""
        r = self.raw.cpu().numpy()
        bad = np.nonzero(r != self.poison)[0].astype(np.int64)
        bad = bad[(bad < self.lo) | (bad >= self.lo + self.nbytes)]
        return bad - self.lo

    def check_guards(self):
        bad = self.stray_writes()
        assert bad.size == 0, f"{self.name}: {bad.size} bytes written outside the array, at offsets {bad[:8]} " \
                              f"(array: 0..{self.nbytes})"

    def numpy(self):
        return self.t.cpu().numpy().view(_NP[self.t.dtype])

    def untouched(self, lo=0, hi=None):
        """True where the bytes [lo, hi) of the view still hold the poison."""
        return bool((self.bytes[lo:hi] == self.poison).all())


def guarded(nbytes, dtype, shift, poison, device="cuda", name="buffer") -> Guarded:
    return Guarded(nbytes, dtype, shift, poison, device, name)


def min_shift(dtype, align=None):
    """The shift that leaves a view at exactly its documented alignment `align` (default: the
    element size) and no better: align mod 2 align."""
    return align if align is not None else torch.empty(0, dtype=dtype).element_size()


def placed(array, shift, device="cuda"):
    """An input array on the device at base + GUARD + shift (inputs carry no poison)."""
    a = np.array(array, order="C")  # a writable copy: torch warns about read-only arrays
    dt ={1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.dtype.itemsize]
    if a.dtype == np.float64:
        dt = torch.float64
    g = Guarded(a.nbytes, dt, shift, 0, device, "input")
    if a.size:
        g.bytes.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
    return g.t.view(a.shape) if a.size else g.t


def mismatches(got, exp, poison, name="output"):
    """None when got == exp element for element; else a message that names the first elements that
    differ and says how many of them still hold the poison (never written)."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    if got.dtype != exp.dtype:
        exp = exp.astype(got.dtype)
    bad = np.nonzero((got != exp).reshape(-1))[0]
    if bad.size == 0:
        return None
    g, e = got.reshape(-1), exp.reshape(-1)
    unwritten = int((g[bad] == poison_value(poison, got.dtype)).sum())
    return (f"{name}: {bad.size} of {g.size} elements differ from the oracle, {unwritten} of them still hold the "
            f"poison 0x{poison:02X} (never written); first at {bad[:6]}: got {g[bad[:6]]} expected {e[bad[:6]]}")


class PoisonRun:
    """The buffers of one of the two runs of a call."""

    def __init__(self, poison, device="cuda"):
        self.poison, self.device, self.bufs = poison, device, {}

    def buf(self, name, count, dtype, align=None) -> torch.Tensor:
        item = torch.empty(0, dtype=dtype).element_size()
        g = Guarded(count * item, dtype, min_shift(dtype, align), self.poison, self.device, name)
        self.bufs[name] = g
        return g.t

    def __getitem__(self, name) -> Guarded:
        return self.bufs[name]

    def expect(self, name, exp, lo=0):
        """Elements [lo, lo + len(exp)) of buffer `name` equal exp."""
        exp = np.asarray(exp).reshape(-1)
        got = self.bufs[name].numpy().reshape(-1)[lo: lo + exp.size]
        msg = mismatches(got, exp, self.poison, name)
        assert msg is None, msg

    def expect_poison(self, name, lo=0, hi=None):
        """Bytes [lo, hi) of buffer `name` were not written."""
        g = self.bufs[name]
        b = g.bytes[lo:hi].cpu().numpy()
        bad = np.nonzero(b != self.poison)[0]
        assert bad.size == 0, f"{name}: {bad.size} bytes written where nothing may be, first at byte {lo + bad[:6]}"

    def expect_head(self, name, exp):
        """Elements [0, len(exp)) of buffer `name` equal exp, and every byte behind them, to the end
        of the array, was not written: a table whose length the device decides."""
        exp = np.asarray(exp).reshape(-1)
        self.expect(name, exp)
        self.expect_poison(name, exp.size * self.bufs[name].t.element_size())

    def expect_rows(self, name, exp, lo, per=1):
        """Rows [lo, lo + len(exp) / per) of buffer `name` (`per` elements a row) equal exp, and the
        rows in front of them and behind them were not written: a slice filled in place."""
        exp = np.asarray(exp).reshape(-1)
        item = self.bufs[name].t.element_size()
        self.expect(name, exp, lo=lo * per)
        self.expect_poison(name, 0, lo * per * item)
        self.expect_poison(name, (lo * per + exp.size) * item)

    def check_guards(self):
        for g in self.bufs.values():
            g.check_guards()


def twice(fn, device="cuda"):
    """fn(run) allocates its outputs and workspaces from `run`, makes the call, synchronises and
    compares with the oracle; it runs once per poison, and every guard band is checked after it."""
    for poison in POISONS:
        run = PoisonRun(poison, device)
        fn(run)
        run.check_guards()


def workspace_history(ws, big, small, fills=(0xFF, 0x00)):
    """The runs of a workspace-contents test on one workspace tensor `ws`: big(ws), then small(ws)
    on what the big call left, then for every fill byte small and big again, each on a workspace
    filled with that byte right before it.  big / small make the call and compare its outputs."""
    big(ws)
    small(ws)  # stale from the larger call
    for fill in fills:
        for call in (small, big):
            ws.fill_(fill)
            call(ws)


def frag_scan_block():
    """kFsBlk of csrc/sbe_codec.hip: the fragments one scan block of the reassembly takes."""
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(os.path.dirname(here), "aeron-cluster-client-cpp_amd", "csrc", "sbe_codec.hip")) as f:
        src = f.read()
    per = int(re.search(r"#define SBE_FS_PER (\d+)", src).group(1))
    threads = int(re.search(r"kFsThreads = (\d+)", src).group(1))
    assert re.search(r"kFsBlk = kFsPer \* kFsThreads", src)
    return per * threads


def reassemble_raw(codec, data, frag_off, flags, out, msg_off, counts, workspace, stream=None):
    """sbe_reassemble_fragments with every output the caller's (the binding allocates counts)."""
    n = int(flags.numel())
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = codec.lib().sbe_reassemble_fragments(
        ctypes.c_void_p(data.data_ptr()), ctypes.c_void_p(frag_off.data_ptr()), ctypes.c_void_p(flags.data_ptr()), n,
        ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(msg_off.data_ptr()), ctypes.c_void_p(counts.data_ptr()),
        ctypes.c_void_p(workspace.data_ptr()), int(workspace.numel()), ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, rc


def reassembled_expected(msgs, carry):
    """(bytes, msg_off [m + 1], counts) of the oracle's messages and carry."""
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b"".join(msgs) + carry, np.uint8), off, np.array([len(msgs), len(carry)], np.uint64)
