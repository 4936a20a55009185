"""CPU: the C ABI of sbe_term_poll: declarations, exports, the struct's field order, the unchanged
ABI version, and every argument check that returns before anything touches a device (fake
pointers, no device)."""
import ctypes
import os
import re

import pytest

import sbe_testlib as T

HEADER = os.path.join(T.ROOT, "include", "sbecodec.h")
EINVAL, ENOSPC = -1, -3
BLK, OUT, OFF, CNT, WS, CARRY = (0x10000000 * k for k in range(1, 7))


class PollOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("msg_off", "counts")]


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(os.path.join(T.PKG, "libsbecodec.so"))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.sbe_term_poll.restype = ctypes.c_int
    L.sbe_term_poll.argtypes = [vp, u64, u64, u64, u64, vp, u64, vp, u64, ctypes.POINTER(PollOut), vp, ctypes.c_size_t, vp]
    L.sbe_term_poll_workspace_size.restype = ctypes.c_size_t
    L.sbe_term_poll_workspace_size.argtypes = [u64, u64]
    L.sbe_term_scan_workspace_size.restype = ctypes.c_size_t
    L.sbe_term_scan_workspace_size.argtypes = [u64]
    L.sbe_abi_version.restype = ctypes.c_int
    return L


def test_header_declares_and_library_exports(lib):
    text = open(HEADER).read()
    for name in ("sbe_term_poll", "sbe_term_poll_workspace_size"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name)
    assert "sbe_term_poll()" in text[: text.index("#ifndef SBECODEC_H")]
    body = text[text.index("typedef struct sbe_term_poll_out"): text.index("} sbe_term_poll_out;")]
    assert re.findall(r"^\s+u?int\d+_t\* (\w+);", body, re.M) == ["msg_off", "counts"]
    assert "#define SBECODEC_ABI_VERSION 8" in text and lib.sbe_abi_version() == 8


def test_workspace_is_monotonic(lib):
    size = lib.sbe_term_poll_workspace_size
    blocks = (0, 32, 32768, 32768 + 32, 1 << 20, 1 << 24, 1 << 30)
    caps = (0, 1, 1000, 1024, 1025, 1 << 20, 1 << 40, (1 << 64) - 1)
    for c in caps:
        sizes = [size(b, c) for b in blocks]
        assert sizes == sorted(sizes), c
    for b in blocks:
        sizes = [size(b, c) for c in caps]
        assert sizes == sorted(sizes), b
        assert size(b, 1) >= lib.sbe_term_scan_workspace_size(b)
    assert size(32, 1) > 0 and size(1 << 20, 10) < size(1 << 20, 10000)


def _call(lib, block=BLK, nbytes=4096, start=0, limit=100, cap=100, carry=None, carry_bytes=0, out=OUT, out_cap=None,
          o="good", ws=WS, ws_bytes=None, msg_off=OFF, counts=CNT):
    t = PollOut(msg_off, counts)
    if ws_bytes is None:
        ws_bytes = lib.sbe_term_poll_workspace_size(nbytes, cap) if nbytes <= 1 << 31 else 1 << 40
    if out_cap is None:
        out_cap = carry_bytes + max(nbytes - start, 0)
    return lib.sbe_term_poll(block, nbytes, start, limit, cap, carry, carry_bytes, out, out_cap,
                             ctypes.byref(t) if o else None, ws, ws_bytes, None)


def test_refuses_what_term_scan_refuses(lib):
    assert _call(lib, nbytes=4096 + 16) == EINVAL
    assert _call(lib, nbytes=4096 + 1) == EINVAL
    assert _call(lib, start=8) == EINVAL
    assert _call(lib, start=4096 + 32) == EINVAL
    assert _call(lib, nbytes=(1 << 30) + 32) == EINVAL
    assert _call(lib, nbytes=1 << 40) == EINVAL
    assert _call(lib, block=BLK + 8) == EINVAL
    assert _call(lib, block=None) == EINVAL
    assert _call(lib, ws=None) == EINVAL


def test_refuses_null_and_misaligned_outputs(lib):
    assert _call(lib, o=None) == EINVAL
    assert _call(lib, msg_off=None) == EINVAL
    assert _call(lib, counts=None) == EINVAL
    assert _call(lib, out=None) == EINVAL
    assert _call(lib, msg_off=OFF + 4) == EINVAL
    assert _call(lib, counts=CNT + 4) == EINVAL
    # whatever the sizes are: a call that would deliver nothing is checked the same
    assert _call(lib, nbytes=0, counts=None) == EINVAL
    assert _call(lib, nbytes=0, out=None) == EINVAL
    assert _call(lib, nbytes=64, start=64, msg_off=OFF + 1) == EINVAL
    assert _call(lib, limit=0, counts=CNT + 4) == EINVAL


def test_refuses_a_bad_carry(lib):
    assert _call(lib, carry=None, carry_bytes=1) == EINVAL
    # 2^31 bytes of output at the most
    assert _call(lib, nbytes=1 << 30, carry=CARRY, carry_bytes=(1 << 30) + 1, ws_bytes=1 << 40) == EINVAL
    assert _call(lib, nbytes=4096, start=4096, carry=CARRY, carry_bytes=(1 << 31) + 1) == EINVAL
    assert _call(lib, nbytes=4096, carry=CARRY, carry_bytes=(1 << 64) - 64) == EINVAL
    # the carry may not overlap out: inside it, across its start, across its end, around it
    n = 4096 + 100
    assert _call(lib, carry=OUT + 10, carry_bytes=100) == EINVAL
    assert _call(lib, carry=OUT - 50, carry_bytes=100) == EINVAL
    assert _call(lib, carry=OUT + n - 1, carry_bytes=100) == EINVAL
    assert _call(lib, carry=OUT - 50, carry_bytes=100, out_cap=8) == EINVAL  # a bad argument wins over a short out
    assert _call(lib, carry=OUT - 1, carry_bytes=n + 2) == EINVAL
    # a larger out_capacity than needed counts whole
    assert _call(lib, carry=OUT + n + 50, carry_bytes=100, out_cap=n + 51) == EINVAL


def test_short_buffers(lib):
    assert _call(lib, out_cap=4095) == ENOSPC
    assert _call(lib, start=64, out_cap=4096 - 65) == ENOSPC
    assert _call(lib, carry=CARRY, carry_bytes=10, out_cap=4096 + 9) == ENOSPC
    assert _call(lib, nbytes=64, start=64, carry=CARRY, carry_bytes=10, out_cap=9) == ENOSPC
    need = lib.sbe_term_poll_workspace_size(4096, 100)
    assert _call(lib, ws_bytes=need - 1) == ENOSPC
    assert _call(lib, ws_bytes=0) == ENOSPC
    assert _call(lib, cap=1 << 20, ws_bytes=lib.sbe_term_poll_workspace_size(4096, 1 << 20) - 1) == ENOSPC
    # a bad argument wins over a short buffer
    assert _call(lib, ws_bytes=0, start=8) == EINVAL
    assert _call(lib, out_cap=0, start=8) == EINVAL
    assert _call(lib, out_cap=0, counts=CNT + 4) == EINVAL
    assert _call(lib, ws_bytes=0, carry=None, carry_bytes=5) == EINVAL
