"""CPU: the C ABI of sbe_term_scan: declarations, exports, code values, the tile, and the argument
checks that return before anything touches a device (fake pointers, no device)."""
import ctypes
import os
import re

import pytest

import sbe_testlib as T

HEADER = os.path.join(T.ROOT, "include", "sbecodec.h")
EINVAL, ENOSPC = -1, -3
BLK, OUT, OFF, FL, SRC, CNT, WS = (0x100000 * k for k in range(1, 8))


class TermOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("frag_off", "flags", "frag_src", "counts")]


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(os.path.join(T.PKG, "libsbecodec.so"))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.sbe_term_scan.restype = ctypes.c_int
    L.sbe_term_scan.argtypes = [vp, u64, u64, u64, u64, vp, ctypes.POINTER(TermOut), vp, ctypes.c_size_t, vp]
    L.sbe_term_scan_workspace_size.restype = ctypes.c_size_t
    L.sbe_term_scan_workspace_size.argtypes = [u64]
    L.sbe_term_scan_tile.restype = ctypes.c_uint32
    L.sbe_abi_version.restype = ctypes.c_int
    return L


def test_header_declares_and_library_exports(lib):
    text = open(HEADER).read()
    for name in ("sbe_term_scan", "sbe_term_scan_tile", "sbe_term_scan_workspace_size"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name)
    assert "sbe_term_scan()" in text[: text.index("#ifndef SBECODEC_H")]
    vals = dict(re.findall(r"#define (SBE_TERM_STOP_\w+) +(\d+)u", text))
    assert {k: int(v) for k, v in vals.items()} == {
        "SBE_TERM_STOP_END": 0, "SBE_TERM_STOP_LIMIT": 1, "SBE_TERM_STOP_UNCOMMITTED": 2, "SBE_TERM_STOP_SHORT": 3,
        "SBE_TERM_STOP_PARTIAL": 4}
    body = text[text.index("typedef struct sbe_term_out"): text.index("} sbe_term_out;")]
    assert re.findall(r"^\s+u?int\d+_t\* (\w+);", body, re.M) == ["frag_off", "flags", "frag_src", "counts"]
    assert "#define SBECODEC_ABI_VERSION 8" in text and lib.sbe_abi_version() == 8


def test_tile_and_workspace(lib):
    t = lib.sbe_term_scan_tile()
    assert t % 32 == 0 and t >= 32
    sizes = [lib.sbe_term_scan_workspace_size(b) for b in (0, 32, t, t + 32, 16 * t, 1 << 30)]
    assert sizes == sorted(sizes) and sizes[1] > 0


def _call(lib, block=BLK, nbytes=4096, start=0, limit=100, cap=100, out=OUT, o="good", ws=WS, ws_bytes=None, **kw):
    t = TermOut(kw.get("frag_off", OFF), kw.get("flags", FL), kw.get("frag_src", SRC), kw.get("counts", CNT))
    if ws_bytes is None:
        ws_bytes = lib.sbe_term_scan_workspace_size(nbytes) if nbytes <= 1 << 31 else 1 << 40
    return lib.sbe_term_scan(block, nbytes, start, limit, cap, out, ctypes.byref(t) if o else None, ws, ws_bytes, None)


def test_refuses_bad_arguments(lib):
    assert _call(lib, o=None) == EINVAL
    for field in ("counts", "frag_off", "flags"):
        assert _call(lib, **{field: None}) == EINVAL, field
        assert _call(lib, nbytes=0, **{field: None}) == EINVAL, field
    assert _call(lib, nbytes=4096 + 16) == EINVAL
    assert _call(lib, nbytes=4096 + 1) == EINVAL
    assert _call(lib, start=8) == EINVAL
    assert _call(lib, start=4096 + 32) == EINVAL
    assert _call(lib, nbytes=(1 << 30) + 32) == EINVAL
    assert _call(lib, nbytes=1 << 40) == EINVAL
    assert _call(lib, block=BLK + 8) == EINVAL
    assert _call(lib, frag_off=OFF + 4) == EINVAL
    assert _call(lib, counts=CNT + 4) == EINVAL
    assert _call(lib, frag_src=SRC + 2) == EINVAL
    assert _call(lib, block=None) == EINVAL
    assert _call(lib, ws=None) == EINVAL
    # misalignment is refused whatever the sizes are
    assert _call(lib, nbytes=0, counts=CNT + 4) == EINVAL
    assert _call(lib, nbytes=64, start=64, frag_off=OFF + 1) == EINVAL


def test_short_workspace(lib):
    need = lib.sbe_term_scan_workspace_size(4096)
    assert _call(lib, ws_bytes=need - 1) == ENOSPC
    assert _call(lib, ws_bytes=0) == ENOSPC
    assert _call(lib, nbytes=1 << 30, ws_bytes=lib.sbe_term_scan_workspace_size(1 << 30) - 1) == ENOSPC
    # a bad argument wins over a short workspace
    assert _call(lib, ws_bytes=0, start=8) == EINVAL
