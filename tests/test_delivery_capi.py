"""CPU: the C ABI of delivery tracking (sbe_inflight_note_keys, sbe_inflight_lookup_keys,
sbe_inflight_reset_values, sbe_delivery_keys): declarations, code values, and argument checks that
return before anything touches a device."""
import ctypes
import os
import re

import pytest

import sbe_testlib as T

HEADER = os.path.join(T.ROOT, "include", "sbecodec.h")
NAMES = ("sbe_inflight_note_keys", "sbe_inflight_lookup_keys", "sbe_inflight_reset_values", "sbe_delivery_keys")
EINVAL, ENOSPC = -1, -3
TABLE, BUF, POS, LEN, CODE, RES, TOT, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000
KEY_OUT = ("msg_pos", "msg_len", "coid_pos", "coid_len", "coid_kind", "oid_pos", "oid_len", "oid_kind", "selected", "totals")
PATHS = ("message", "message.message", "message.message.client_order_id", "message.message.order_id",
         "message.message.order_details", "message.message.order_details.client_order_id", "message.order_details",
         "message.order_details.client_order_id", "uuid")


class Decoded(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("status", "flags", "hdr", "ts", "view_off", "view_len", "seq")]


class JsonOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("doc", "root_kind", "kind", "off", "len")]


class KeyOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in KEY_OUT]


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(os.path.join(T.PKG, "libsbecodec.so"))
    vp, u64, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t
    for name in NAMES[:2]:
        f = getattr(L, name)
        f.restype = ctypes.c_int
        f.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, vp, vp, sz, vp]
    L.sbe_inflight_reset_values.restype = ctypes.c_int
    L.sbe_inflight_reset_values.argtypes = [vp, vp]
    L.sbe_delivery_keys.restype = ctypes.c_int
    L.sbe_delivery_keys.argtypes = [vp, u64, ctypes.POINTER(Decoded), vp, ctypes.POINTER(JsonOut), ctypes.POINTER(KeyOut), vp]
    L.sbe_inflight_workspace_size.restype = sz
    L.sbe_inflight_workspace_size.argtypes = [u64]
    return L


def test_header_declares_and_library_exports(lib):
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name)
    table = text[: text.index("#ifndef SBECODEC_H")]
    for name in ("sbe_inflight_note_keys()", "sbe_inflight_lookup_keys()", "sbe_delivery_keys()"):
        assert name in table
    assert "typedef struct sbe_delivery_key_out" in text and "#define SBE_NO_KEY 0xFFFFFFFFu" in text
    assert [int(v) for v in re.findall(r"#define SBE_DLV_(?:NONE|NEW|AGAIN|LONG|FULL) +(\d+)u", text)] == [0, 1, 2, 3, 4]
    assert [int(v) for v in re.findall(r"#define SBE_SENT_(?:NONE|UNKNOWN|FIRST|REPEAT|LONG) +(\d+)u", text)] == [0, 1, 2, 3, 4]
    assert "+32 u64 answered" in text
    # the nine paths are the documented contract of `ids`, in the order of the host's order_id_paths()
    doc = text[text.index("#define SBE_DLV_PATHS") - 700: text.index("#define SBE_DLV_PATHS")]
    assert re.findall(r"\b(\d) ((?:message|uuid)[a-z_.]*)", doc) == [(str(i), p) for i, p in enumerate(PATHS)]
    assert "#define SBE_DLV_PATHS 9u" in text
    # the fields of sbe_delivery_key_out, in order
    body = text[text.index("typedef struct sbe_delivery_key_out"): text.index("} sbe_delivery_key_out;")]
    assert re.findall(r"^\s+u?int\d+_t\* (\w+);", body, re.M) == list(KEY_OUT)


def test_existing_codes_and_abi_version_are_unchanged(lib):
    text = open(HEADER).read()
    assert [int(v) for v in re.findall(r"#define SBE_INF_[A-Z_]+ (\d+)u", text)] == [0, 1, 2, 3, 4]
    assert [int(v) for v in re.findall(r"#define SBE_ACK_(?:NONE|MATCHED|UNMATCHED|LONG_ID) (\d+)u", text)] == [0, 1, 2, 3]
    lib.sbe_abi_version.restype = ctypes.c_int
    assert lib.sbe_abi_version() == 8


def _keys(lib, fn, table=TABLE, buf=BUF, pos=POS, ln=LEN, n=4, code=CODE, res=RES, totals=TOT, ws=WS, ws_bytes=1 << 20):
    return getattr(lib, fn)(table, buf, 1 << 16, pos, ln, n, code, res, totals, ws, ws_bytes, None)


@pytest.mark.parametrize("fn,res_align", [("sbe_inflight_note_keys", 4), ("sbe_inflight_lookup_keys", 8)])
def test_key_calls_refuse_bad_arguments(lib, fn, res_align):
    """The pointers are never dereferenced here: every call is refused first."""
    for name in ("table", "buf", "pos", "ln", "code", "res", "ws"):
        assert _keys(lib, fn, **{name: None}) == EINVAL, name
    assert _keys(lib, fn, table=TABLE + 32) == EINVAL
    assert _keys(lib, fn, pos=POS + 4) == EINVAL
    assert _keys(lib, fn, ln=LEN + 2) == EINVAL
    assert _keys(lib, fn, res=RES + res_align // 2) == EINVAL
    assert _keys(lib, fn, totals=TOT + 4) == EINVAL
    assert _keys(lib, fn, ws=WS + 2) == EINVAL
    assert _keys(lib, fn, n=2 ** 32) == EINVAL
    assert _keys(lib, fn, n=1000, ws_bytes=lib.sbe_inflight_workspace_size(1000) - 1) == ENOSPC
    assert _keys(lib, fn, ws_bytes=8) == ENOSPC
    assert _keys(lib, fn, n=0, totals=None) == 0  # no totals to zero: nothing launched
    assert _keys(lib, fn, n=0, totals=None, buf=None, pos=None, ln=None, code=None, res=None, ws=None) == 0
    assert _keys(lib, fn, n=0, table=None) == EINVAL


def test_reset_values_refuses_bad_tables(lib):
    assert lib.sbe_inflight_reset_values(None, None) == EINVAL
    assert lib.sbe_inflight_reset_values(TABLE + 8, None) == EINVAL


def _delivery_keys(lib, rec=0x90000, n=4, dec="good", ids="good", out="good", **kw):
    d = Decoded(0xA0000, 0xB0000, None, None, 0xC0000, 0xD0000, None)
    j = JsonOut(0xE0000, 0xF0000, 0x100000, 0x110000, 0x120000)
    o = KeyOut(*(0x200000 + 0x10000 * i for i in range(len(KEY_OUT))))
    for k, v in kw.items():
        setattr(next(s for s in (o, j, d) if hasattr(s, k)), k, v)
    return lib.sbe_delivery_keys(rec, n, ctypes.byref(d) if dec else None, None, ctypes.byref(j) if ids else None,
                                 ctypes.byref(o) if out else None, None)


def test_delivery_keys_refuses_bad_arguments(lib):
    assert _delivery_keys(lib, rec=None) == EINVAL
    assert _delivery_keys(lib, dec=None) == EINVAL
    assert _delivery_keys(lib, ids=None) == EINVAL
    assert _delivery_keys(lib, out=None) == EINVAL
    assert _delivery_keys(lib, out=None, n=0) == EINVAL
    assert _delivery_keys(lib, n=0, totals=None) == EINVAL
    for field in ("status", "view_off", "view_len", "doc", "root_kind", "kind", "off", "len") + KEY_OUT:
        assert _delivery_keys(lib, **{field: None}) == EINVAL, field
    assert _delivery_keys(lib, rec=0x90004) == EINVAL
    assert _delivery_keys(lib, view_off=0xC0002) == EINVAL
    assert _delivery_keys(lib, view_len=0xD0001) == EINVAL
    assert _delivery_keys(lib, off=0x110002) == EINVAL
    assert _delivery_keys(lib, len=0x120002) == EINVAL
    for i, field in enumerate(KEY_OUT):
        if field.endswith("pos") or field == "totals":
            assert _delivery_keys(lib, **{field: 0x200000 + 0x10000 * i + 4}) == EINVAL, field
        elif field.endswith("len"):
            assert _delivery_keys(lib, **{field: 0x200000 + 0x10000 * i + 2}) == EINVAL, field
    assert _delivery_keys(lib, n=2 ** 32) == EINVAL
