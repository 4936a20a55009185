"""CPU: the C ABI of sbe_term_append: declarations, exports, code values, struct field order, the
frame-length function against the Python restatement, and the argument checks that return before
anything touches a device (fake pointers, no device)."""
import ctypes
import os
import re

import pytest

import sbe_testlib as T
import termappend_lib as A

HEADER = os.path.join(T.ROOT, "include", "sbecodec.h")
EINVAL, ENOSPC = -1, -3
IN, OFF, BLK, TAIL, CNT, WS = (0x100000 * k for k in range(1, 7))


class TermHeader(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("session_id", "stream_id", "term_id", "term_offset_base")] + [("version", ctypes.c_uint8)]


class AppendOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("rec_tail", "counts")]


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(os.path.join(T.PKG, "libsbecodec.so"))
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    L.sbe_term_append.restype = ctypes.c_int
    L.sbe_term_append.argtypes = [vp, u64, vp, u64, vp, u64, u64, u64, u32, u64, ctypes.POINTER(TermHeader),
                                  ctypes.POINTER(AppendOut), vp, ctypes.c_size_t, vp]
    L.sbe_term_append_workspace_size.restype = ctypes.c_size_t
    L.sbe_term_append_workspace_size.argtypes = [u64]
    L.sbe_term_append_tile.restype = u32
    L.sbe_term_frames_length.restype = u64
    L.sbe_term_frames_length.argtypes = [u64, u32]
    L.sbe_abi_version.restype = ctypes.c_int
    return L


def test_header_declares_and_library_exports(lib):
    text = open(HEADER).read()
    for name in ("sbe_term_append", "sbe_term_append_tile", "sbe_term_append_workspace_size", "sbe_term_frames_length"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name)
    assert "sbe_term_append()" in text[: text.index("#ifndef SBECODEC_H")]
    vals = dict(re.findall(r"#define (SBE_TERM_APPEND_\w+) +(\d+)u", text))
    assert {k: int(v) for k, v in vals.items()} == {
        "SBE_TERM_APPEND_END": 0, "SBE_TERM_APPEND_LIMIT": 1, "SBE_TERM_APPEND_TRIPPED": 2, "SBE_TERM_APPEND_TOO_LONG": 3,
        "SBE_TERM_APPEND_BAD_RECORD": 4}
    assert (A.END, A.LIMIT, A.TRIPPED, A.TOO_LONG, A.BAD_RECORD) == (0, 1, 2, 3, 4)
    body = text[text.index("typedef struct sbe_term_header"): text.index("} sbe_term_header;")]
    assert re.findall(r"^\s+(u?int\d+_t) (\w+);", body, re.M) == [
        ("int32_t", "session_id"), ("int32_t", "stream_id"), ("int32_t", "term_id"), ("int32_t", "term_offset_base"),
        ("uint8_t", "version")]
    body = text[text.index("typedef struct sbe_term_append_out"): text.index("} sbe_term_append_out;")]
    assert re.findall(r"^\s+uint64_t\* (\w+);", body, re.M) == ["rec_tail", "counts"]
    assert "#define SBECODEC_ABI_VERSION 8" in text and lib.sbe_abi_version() == 8


def test_python_binding_names_the_codes():
    src = open(os.path.join(T.PKG, "sbecodec.py")).read()
    assert "TERM_APPEND_END, TERM_APPEND_LIMIT, TERM_APPEND_TRIPPED, TERM_APPEND_TOO_LONG, TERM_APPEND_BAD_RECORD = range(5)" in src
    for name in ("def term_append(", "def term_append_tile(", "def term_frames_length(", "class TermHeader"):
        assert name in src, name


def test_tile_and_workspace(lib):
    t = lib.sbe_term_append_tile()
    assert t % 32 == 0 and t >= 32
    sizes = [lib.sbe_term_append_workspace_size(n) for n in (0, 1, 1023, 1024, 1025, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[1] >= 8


def test_frames_length_against_the_restatement(lib):
    for mtu in A.MTUS:
        maxp = mtu - 32
        lengths = list(range(0, 3 * mtu + 2)) + [k * maxp + d for k in (7, 100, 4097) for d in (-1, 0, 1, 31, 32, 33)]
        lengths += [1 << 24, (1 << 30) - 1, 1 << 30]
        for n in lengths:
            assert lib.sbe_term_frames_length(n, mtu) == A.required(n, mtu), (mtu, n)
    for mtu in (0, 32, 63, 65, 100, 1400, 65536, 65505, 65536 + 64):
        assert lib.sbe_term_frames_length(10, mtu) == 0, mtu
    assert lib.sbe_term_frames_length(10, 65504) == 64


def _call(lib, data=IN, in_bytes=4096, rec_off=OFF, n=10, block=BLK, nbytes=4096, start=0, limit=(1 << 64) - 1, mtu=1408,
          max_len=1 << 20, hdr="good", o="good", ws=WS, ws_bytes=None, rec_tail=TAIL, counts=CNT):
    h = TermHeader(1, 2, 3, 0, 1)
    out = AppendOut(rec_tail, counts)
    if ws_bytes is None:
        ws_bytes = lib.sbe_term_append_workspace_size(n)
    return lib.sbe_term_append(data, in_bytes, rec_off, n, block, nbytes, start, limit, mtu, max_len,
                               ctypes.byref(h) if hdr else None, ctypes.byref(out) if o else None, ws, ws_bytes, None)


def test_refuses_bad_arguments(lib):
    assert _call(lib, hdr=None) == EINVAL
    assert _call(lib, o=None) == EINVAL
    assert _call(lib, counts=None) == EINVAL
    for n in (0, 10):  # whatever n is
        assert _call(lib, n=n, hdr=None) == EINVAL
        assert _call(lib, n=n, o=None) == EINVAL
        assert _call(lib, n=n, counts=None) == EINVAL
        assert _call(lib, n=n, nbytes=4096 + 16) == EINVAL
        assert _call(lib, n=n, nbytes=4096 + 1) == EINVAL
        assert _call(lib, n=n, start=8) == EINVAL
        assert _call(lib, n=n, start=4096 + 32) == EINVAL
        assert _call(lib, n=n, nbytes=(1 << 30) + 32, start=0) == EINVAL
        assert _call(lib, n=n, nbytes=1 << 40) == EINVAL
        for mtu in (0, 32, 48, 1400, 65536, 65504 + 32):
            assert _call(lib, n=n, mtu=mtu) == EINVAL, mtu
        assert _call(lib, n=n, max_len=(1 << 30) + 1) == EINVAL
        assert _call(lib, n=n, block=BLK + 8) == EINVAL
        assert _call(lib, n=n, rec_off=OFF + 4) == EINVAL
        assert _call(lib, n=n, rec_tail=TAIL + 4) == EINVAL
        assert _call(lib, n=n, counts=CNT + 4) == EINVAL
    for name in ("rec_off", "data", "block", "ws"):
        assert _call(lib, **{name: None}) == EINVAL, name


def test_short_workspace(lib):
    need = lib.sbe_term_append_workspace_size(10)
    assert _call(lib, ws_bytes=need - 1) == ENOSPC
    assert _call(lib, ws_bytes=0) == ENOSPC
    big = 1 << 20
    assert _call(lib, n=big, ws_bytes=lib.sbe_term_append_workspace_size(big) - 1) == ENOSPC
    # a bad argument wins over a short workspace
    assert _call(lib, ws_bytes=0, start=8) == EINVAL
    assert _call(lib, ws_bytes=0, mtu=100) == EINVAL
    assert _call(lib, ws_bytes=0, counts=CNT + 4) == EINVAL
