"""CPU: the C ABI of ack correlation (sbe_inflight_*): sizes, and argument checks that return
before anything touches a device."""
import ctypes
import os
import re

import pytest

import sbe_testlib as T

HEADER = os.path.join(T.ROOT, "include", "sbecodec.h")
NAMES = ("sbe_inflight_table_size", "sbe_inflight_init", "sbe_inflight_workspace_size", "sbe_inflight_remember",
         "sbe_inflight_match_acks", "sbe_inflight_rehash")
EINVAL, ENOSPC = -1, -3
TABLE, ARENA, OFF, LEN, TS, WS, IN, REC = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000


class Decoded(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("status", "flags", "hdr", "ts", "view_off", "view_len", "seq")]


class AckOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("code", "base_ns", "counts")]


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(os.path.join(T.PKG, "libsbecodec.so"))
    vp, u64, u32, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_size_t
    L.sbe_inflight_table_size.restype = sz
    L.sbe_inflight_table_size.argtypes = [u64]
    L.sbe_inflight_workspace_size.restype = sz
    L.sbe_inflight_workspace_size.argtypes = [u64]
    L.sbe_inflight_init.restype = ctypes.c_int
    L.sbe_inflight_init.argtypes = [vp, sz, u64, u32, vp]
    L.sbe_inflight_remember.restype = ctypes.c_int
    L.sbe_inflight_remember.argtypes = [vp, vp, vp, vp, u32, vp, u64, vp, u64, vp, vp, sz, vp]
    L.sbe_inflight_match_acks.restype = ctypes.c_int
    L.sbe_inflight_match_acks.argtypes = [vp, vp, vp, u64, ctypes.POINTER(Decoded), ctypes.POINTER(AckOut), vp, sz, vp]
    L.sbe_inflight_rehash.restype = ctypes.c_int
    L.sbe_inflight_rehash.argtypes = [vp, vp, vp]
    return L


def test_header_declares_and_library_exports(lib):
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name)
    table = text[: text.index("#ifndef SBECODEC_H")]
    assert "sbe_inflight_remember()" in table and "sbe_inflight_match_acks()" in table
    assert "typedef struct sbe_ack_out" in text and "#define SBE_INFLIGHT_KEY_MAX 40u" in text
    assert [int(v) for v in re.findall(r"#define SBE_INF_[A-Z_]+ (\d+)u", text)] == [0, 1, 2, 3, 4]
    assert [int(v) for v in re.findall(r"#define SBE_ACK_(?:NONE|MATCHED|UNMATCHED|LONG_ID) (\d+)u", text)] == [0, 1, 2, 3]
    lib.sbe_abi_version.restype = ctypes.c_int
    assert lib.sbe_abi_version() == 8


@pytest.mark.parametrize("capacity", [0, 1, 32, 63, 65, 96, 1000, 2 ** 31 + 1, 2 ** 32, 2 ** 40])
def test_table_size_refuses_bad_capacities(lib, capacity):
    assert lib.sbe_inflight_table_size(capacity) == 0


@pytest.mark.parametrize("capacity", [64, 128, 1 << 20, 1 << 31])
def test_table_size(lib, capacity):
    assert lib.sbe_inflight_table_size(capacity) == 64 + 64 * capacity


def test_workspace_size(lib):
    assert 0 < lib.sbe_inflight_workspace_size(0) <= 64
    for n in (1, 1000, 10 ** 6):
        assert 4 * n <= lib.sbe_inflight_workspace_size(n) <= 8 * n + 64


def test_init_refuses_bad_arguments(lib):
    size = 64 + 64 * 64
    assert lib.sbe_inflight_init(None, size, 64, 0, None) == EINVAL
    assert lib.sbe_inflight_init(TABLE + 32, size, 64, 0, None) == EINVAL  # 64-byte alignment
    assert lib.sbe_inflight_init(TABLE, size, 65, 0, None) == EINVAL
    assert lib.sbe_inflight_init(TABLE, size, 32, 0, None) == EINVAL
    assert lib.sbe_inflight_init(TABLE, size - 1, 64, 0, None) == EINVAL
    assert lib.sbe_inflight_init(TABLE, size, 64, 31, None) == EINVAL


def _remember(lib, table=TABLE, arena=ARENA, off=OFF, ln=LEN, stride=1, ts=TS, n=4, ws=WS, ws_bytes=1 << 20):
    return lib.sbe_inflight_remember(table, arena, off, ln, stride, ts, 0, None, n, None, ws, ws_bytes, None)


def test_remember_refuses_bad_arguments(lib):
    """The pointers are never dereferenced here: every call is refused first."""
    assert _remember(lib, table=None) == EINVAL
    assert _remember(lib, table=TABLE + 16) == EINVAL
    assert _remember(lib, arena=None) == EINVAL
    assert _remember(lib, off=None) == EINVAL
    assert _remember(lib, ln=None) == EINVAL
    assert _remember(lib, ws=None) == EINVAL
    assert _remember(lib, stride=0) == EINVAL
    assert _remember(lib, off=OFF + 2) == EINVAL
    assert _remember(lib, ln=LEN + 1) == EINVAL
    assert _remember(lib, ts=TS + 4) == EINVAL
    assert _remember(lib, ws=WS + 2) == EINVAL
    assert _remember(lib, n=2 ** 32) == EINVAL
    assert _remember(lib, ws_bytes=8) == ENOSPC
    assert _remember(lib, n=0) == 0  # nothing to do, nothing launched
    assert _remember(lib, n=0, table=None) == EINVAL


def _match(lib, table=TABLE, data=IN, rec=REC, n=4, dec="good", out="good", ws=WS, ws_bytes=1 << 20, **kw):
    d = Decoded(0x90000, 0xA0000, 0xB0000, 0xC0000, 0xD0000, 0xE0000, None)
    o = AckOut(0xF0000, 0x100000, 0x110000)
    for k, v in kw.items():
        setattr(d if hasattr(d, k) else o, k, v)
    return lib.sbe_inflight_match_acks(table, data, rec, n, ctypes.byref(d) if dec else None,
                                       ctypes.byref(o) if out else None, ws, ws_bytes, None)


def test_match_refuses_bad_arguments(lib):
    assert _match(lib, table=None) == EINVAL
    assert _match(lib, table=TABLE + 8) == EINVAL
    assert _match(lib, data=None) == EINVAL
    assert _match(lib, rec=None) == EINVAL
    assert _match(lib, dec=None) == EINVAL
    assert _match(lib, out=None) == EINVAL
    assert _match(lib, out=None, n=0) == EINVAL
    assert _match(lib, ws=None) == EINVAL
    for field in ("status", "ts", "view_off", "view_len", "code", "base_ns"):
        assert _match(lib, **{field: None}) == EINVAL, field
    assert _match(lib, rec=REC + 4) == EINVAL
    assert _match(lib, ts=0xC0004) == EINVAL
    assert _match(lib, view_off=0xD0002) == EINVAL
    assert _match(lib, view_len=0xE0001) == EINVAL
    assert _match(lib, base_ns=0x100004) == EINVAL
    assert _match(lib, counts=0x110004) == EINVAL
    assert _match(lib, ws=WS + 1) == EINVAL
    assert _match(lib, n=2 ** 32) == EINVAL
    assert _match(lib, ws_bytes=4) == ENOSPC
    assert _match(lib, n=0, counts=None) == 0  # no counts to initialise: nothing launched


def test_rehash_refuses_bad_arguments(lib):
    assert lib.sbe_inflight_rehash(None, TABLE, None) == EINVAL
    assert lib.sbe_inflight_rehash(TABLE, None, None) == EINVAL
    assert lib.sbe_inflight_rehash(TABLE, TABLE, None) == EINVAL
    assert lib.sbe_inflight_rehash(TABLE + 32, 2 * TABLE, None) == EINVAL
    assert lib.sbe_inflight_rehash(TABLE, 2 * TABLE + 8, None) == EINVAL
