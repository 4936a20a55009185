"""CPU: the C ABI of sbe_order_select: declarations, code values, the window, and argument checks
that return before anything touches a device."""
import ctypes
import os
import re

import pytest

import sbe_testlib as T

HEADER = os.path.join(T.ROOT, "include", "sbecodec.h")
EINVAL = -1
IN, REC, ST, FL, HDR, VO, VL, PRED, SEL, CLS, TOT = (0x10000 * k for k in range(1, 12))


class Decoded(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("status", "flags", "hdr", "ts", "view_off", "view_len", "seq")]


class SelectOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("pred", "select", "topic_class", "totals")]


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(os.path.join(T.PKG, "libsbecodec.so"))
    vp = ctypes.c_void_p
    L.sbe_order_select.restype = ctypes.c_int
    L.sbe_order_select.argtypes = [vp, vp, ctypes.c_uint64, ctypes.POINTER(Decoded), ctypes.POINTER(SelectOut), vp]
    L.sbe_order_select_window.restype = ctypes.c_uint32
    L.sbe_abi_version.restype = ctypes.c_int
    return L


def test_header_declares_and_library_exports(lib):
    text = open(HEADER).read()
    for name in ("sbe_order_select", "sbe_order_select_window"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name)
    assert "sbe_order_select()" in text[: text.index("#ifndef SBECODEC_H")]
    vals = dict(re.findall(r"#define (SBE_(?:PR|TC)_\w+) +(0x[0-9a-f]+|\d+)u", text))
    assert {k: int(v, 0) for k, v in vals.items()} == {
        "SBE_PR_SESSION_EVENT": 1, "SBE_PR_TOPIC_MESSAGE": 2, "SBE_PR_ACKNOWLEDGMENT": 4, "SBE_PR_ORDER_MESSAGE": 8,
        "SBE_TC_UNKNOWN": 0, "SBE_TC_ORDERS": 1, "SBE_TC_CONTROL": 2}
    body = text[text.index("typedef struct sbe_select_out"): text.index("} sbe_select_out;")]
    assert re.findall(r"^\s+u?int\d+_t\* (\w+);", body, re.M) == ["pred", "select", "topic_class", "totals"]
    assert "#define SBECODEC_ABI_VERSION 8" in text and lib.sbe_abi_version() == 8


def test_window(lib):
    w = lib.sbe_order_select_window()
    assert w % 16 == 0 and w >= 4096


def _call(lib, n=4, inp=IN, rec=REC, dec="good", out="good", **kw):
    d = Decoded(kw.get("status", ST), kw.get("flags", FL), kw.get("hdr", HDR), kw.get("ts", None),
                kw.get("view_off", VO), kw.get("view_len", VL), None)
    o = SelectOut(kw.get("pred", PRED), kw.get("select", SEL), kw.get("topic_class", CLS), kw.get("totals", TOT))
    return lib.sbe_order_select(inp, rec, n, ctypes.byref(d) if dec else None, ctypes.byref(o) if out else None, None)


def test_refuses_bad_arguments(lib):
    assert _call(lib, inp=None) == EINVAL
    assert _call(lib, rec=None) == EINVAL
    assert _call(lib, dec=None) == EINVAL
    assert _call(lib, out=None) == EINVAL
    assert _call(lib, out=None, n=0) == EINVAL
    assert _call(lib, n=0, totals=None) == EINVAL
    assert _call(lib, n=0, totals=TOT + 4) == EINVAL
    for field in ("status", "flags", "hdr", "view_off", "view_len", "pred", "totals"):
        assert _call(lib, **{field: None}) == EINVAL, field
    assert _call(lib, rec=REC + 4) == EINVAL
    assert _call(lib, totals=TOT + 4) == EINVAL
    assert _call(lib, hdr=HDR + 1) == EINVAL
    assert _call(lib, view_off=VO + 2) == EINVAL
    assert _call(lib, view_len=VL + 1) == EINVAL
    assert _call(lib, n=2 ** 32) == EINVAL
