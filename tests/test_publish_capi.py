"""CPU: the C ABI of the fused publish path (sbe_publish_orders_*): declared in the header, exported,
argument checks that return before any device call, the workspace bound and the ABI version."""
import ctypes
import os
import re

import pytest

import sbe_testlib as T

HEADER = os.path.join(T.ROOT, "include", "sbecodec.h")
NAMES = ("sbe_publish_orders_workspace_size", "sbe_publish_orders_output_bound", "sbe_publish_orders_batch")


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(os.path.join(T.PKG, "libsbecodec.so"))
    vp, u64, u32, i64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
    L.sbe_publish_orders_workspace_size.restype = ctypes.c_size_t
    L.sbe_publish_orders_workspace_size.argtypes = [u64]
    L.sbe_publish_orders_output_bound.restype = u64
    L.sbe_publish_orders_output_bound.argtypes = [u64, u64, u32, ctypes.c_int]
    L.sbe_publish_orders_batch.restype = ctypes.c_int
    L.sbe_publish_orders_batch.argtypes = [vp, vp, u64, vp, u32, vp, u64, u32, ctypes.c_int, i64, i64, vp, u64, vp, vp,
                                           vp, vp, ctypes.c_size_t, vp]
    return L


def test_header_declares_and_library_exports(lib):
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name)
    assert "sbe_publish_orders_batch()" in text[: text.index("#ifndef SBECODEC_H")]  # the opening table
    assert "typedef struct sbe_order_checks" in text
    codes = [int(m) for m in re.findall(r"#define SBE_PUB_INVALID_[A-Z_]+ (\d+)u\s+/\* \"", text)]
    assert codes == list(range(16, 28))
    enc = [int(m) for m in re.findall(r"#define SBE_ENC_(?:OK|E109_\w+|OVERFLOW) (\d+)u", text)]
    assert not set(codes) & set(enc)


def test_abi_version_unchanged(lib):
    assert lib.sbe_abi_version() == 8


@pytest.mark.parametrize("n", [0, 1, 10 ** 6])
def test_workspace_bound(lib, n):
    assert lib.sbe_publish_orders_workspace_size(n) <= 64 * n + 65536


def _call(lib, orders, out_off, flags=0, n=4, out=0x1000, topic=0x2000, ws=0x3000, ws_bytes=1 << 20, checks=None):
    return lib.sbe_publish_orders_batch(orders, checks, n, topic, 6, None, 0, flags, 1, 0, 0, out, 1 << 16, out_off,
                                        None, None, ws, ws_bytes, None)


def test_bad_arguments_return_before_any_device_call(lib):
    """The pointers are never dereferenced on the device here: every call is refused first."""
    class Batch(ctypes.Structure):
        _fields_ = [(k, ctypes.c_void_p) for k in ("arena", "str_off", "str_len", "customer_id", "timestamp", "quantity")]

    good = Batch(0x10000, None, 0x20000, 0x30000, 0x40000, 0x50000)
    off = 0x60000
    EINVAL, ENOSPC = -1, -3
    assert _call(lib, None, off) == EINVAL                                  # null batch
    assert _call(lib, ctypes.byref(good), None) == EINVAL                   # null out_off
    assert _call(lib, ctypes.byref(Batch(0x10000, None, None, 0x30000, 0x40000, 0x50000)), off) == EINVAL
    assert _call(lib, ctypes.byref(good), off, flags=T.ENC_PUBLISH_TOPIC) == EINVAL
    assert _call(lib, ctypes.byref(good), off, flags=T.ENC_PUBLISH_TOPIC | T.ENC_REF_TRUNCATE8) == EINVAL
    assert _call(lib, ctypes.byref(good), off + 4) == EINVAL                # misaligned out_off
    assert _call(lib, ctypes.byref(good), off, out=0x1008) == EINVAL        # misaligned out
    assert _call(lib, ctypes.byref(good), off, topic=None) == EINVAL        # topic_len without a topic
    assert _call(lib, ctypes.byref(good), off, ws=None) == EINVAL
    assert _call(lib, ctypes.byref(good), off, ws_bytes=16) == ENOSPC
    checks = Batch(0x70000, None, None, 0x80000, 0x90000, 0xa0000)          # checks without str_len
    assert _call(lib, ctypes.byref(good), off, checks=ctypes.byref(checks)) == EINVAL
