"""CPU: the C ABI of the delivery reports (sbe_inflight_list_keys, sbe_latency_log_init,
sbe_latency_append, sbe_latency_report and their size functions): declarations, constants, sizes,
and argument checks that return before anything touches a device."""
import ctypes
import os
import re

import pytest

import sbe_testlib as T

HEADER = os.path.join(T.ROOT, "include", "sbecodec.h")
NAMES = ("sbe_inflight_list_workspace_size", "sbe_inflight_list_keys", "sbe_latency_log_size", "sbe_latency_log_init",
         "sbe_latency_append_workspace_size", "sbe_latency_append", "sbe_latency_report_workspace_size",
         "sbe_latency_report")
EINVAL, ENOSPC = -1, -3
TABLE, OTHER, LOG, CODE, VALUE, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
LIST_OUT = ("count", "key", "len", "value", "answered")
REPORT_OUT = ("count", "stats", "pct_value", "pct_index", "sorted", "order")
IN_OTHER, NOT_IN_OTHER, ANSWERED, UNANSWERED = 1, 2, 4, 8
PCT7 = (75.0, 80.0, 90.0, 95.0, 99.0, 99.9, 99.99)


class ListOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in LIST_OUT]


class ReportOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in REPORT_OUT]


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(os.path.join(T.PKG, "libsbecodec.so"))
    vp, u32, u64, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
    L.sbe_inflight_list_workspace_size.restype = sz
    L.sbe_inflight_list_workspace_size.argtypes = [u32]
    L.sbe_inflight_list_keys.restype = ctypes.c_int
    L.sbe_inflight_list_keys.argtypes = [vp, vp, u32, u64, u32, ctypes.POINTER(ListOut), vp, sz, vp]
    for name in ("sbe_latency_log_size", "sbe_latency_append_workspace_size", "sbe_latency_report_workspace_size"):
        getattr(L, name).restype = sz
        getattr(L, name).argtypes = [u64]
    L.sbe_latency_log_init.restype = ctypes.c_int
    L.sbe_latency_log_init.argtypes = [vp, sz, u64, vp]
    L.sbe_latency_append.restype = ctypes.c_int
    L.sbe_latency_append.argtypes = [vp, vp, vp, u64, u64, u64, u64, vp, sz, vp]
    L.sbe_latency_report.restype = ctypes.c_int
    L.sbe_latency_report.argtypes = [vp, ctypes.POINTER(ctypes.c_double), u32, ctypes.POINTER(ReportOut), vp, sz, vp]
    return L


def test_header_declares_and_library_exports(lib):
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name)
    table = text[: text.index("#ifndef SBECODEC_H")]
    for name in ("sbe_inflight_list_keys()", "sbe_latency_append()", "sbe_latency_report()"):
        assert name in table
    for lines in (":130-204", ":206-274", ":276-353"):
        assert lines in table
    # the new section follows delivery tracking
    assert text.index("delivery tracking ====") < text.index("delivery reports ====") < text.index("fragment reassembly ====")
    assert "#define SBE_LIST_MAX 64u" in text and "#define SBE_LAT_MAX_PCT 16u" in text
    flags = re.findall(r"#define SBE_LIST_(IN_OTHER|NOT_IN_OTHER|ANSWERED|UNANSWERED) +0x(\d)u", text)
    assert flags == [("IN_OTHER", "1"), ("NOT_IN_OTHER", "2"), ("ANSWERED", "4"), ("UNANSWERED", "8")]
    for struct, fields in (("sbe_key_list_out", LIST_OUT), ("sbe_latency_report_out", REPORT_OUT)):
        body = text[text.index("typedef struct %s" % struct): text.index("} %s;" % struct)]
        assert re.findall(r"^\s+u?int\d+_t\* (\w+);", body, re.M) == list(fields)


def test_abi_version_is_unchanged(lib):
    assert "#define SBECODEC_ABI_VERSION 8\n" in open(HEADER).read()
    lib.sbe_abi_version.restype = ctypes.c_int
    assert lib.sbe_abi_version() == 8


def test_size_functions(lib):
    for cap in (1, 8, 1000, 2 ** 20, 2 ** 31):
        assert lib.sbe_latency_log_size(cap) == 64 + 16 * cap
        # two (u64 key, u32 position) buffers at the least
        assert lib.sbe_latency_report_workspace_size(cap) >= 24 * cap
    for cap in (0, 2 ** 31 + 1, 2 ** 40, 2 ** 64 - 1):
        assert lib.sbe_latency_log_size(cap) == 0
        assert lib.sbe_latency_report_workspace_size(cap) == 0
    sizes = [lib.sbe_latency_report_workspace_size(c) for c in (1, 2048, 2049, 70000, 2 ** 20)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    # the list workspace depends on the limit alone: 48 B a candidate per workgroup
    w = [lib.sbe_inflight_list_workspace_size(k) for k in range(65)]
    assert w[0] > 0 and all(b > a for a, b in zip(w, w[1:])) and (w[64] - w[0]) % (64 * 48) == 0
    assert lib.sbe_inflight_list_workspace_size(65) == 0 and lib.sbe_inflight_list_workspace_size(2 ** 32 - 1) == 0
    a = [lib.sbe_latency_append_workspace_size(n) for n in (0, 1, 255, 256, 257, 70000, 2 ** 32 - 1)]
    assert a[0] == a[1] > 0 and a == sorted(a) and a[-1] < 2 ** 32 // 64


def _list(lib, table=TABLE, other=OTHER, flags=NOT_IN_OTHER, min_value=0, limit=10, out="good", ws=WS, ws_bytes=1 << 23, **kw):
    o = ListOut(*(0x100000 + 0x10000 * i for i in range(len(LIST_OUT))))
    for k, v in kw.items():
        setattr(o, k, v)
    return lib.sbe_inflight_list_keys(table, other, flags, min_value, limit, ctypes.byref(o) if out else None, ws, ws_bytes, None)


def test_list_keys_refuses_bad_arguments(lib):
    """The pointers are never dereferenced here: every call is refused first."""
    assert _list(lib, table=None) == EINVAL
    assert _list(lib, out=None) == EINVAL
    assert _list(lib, count=None) == EINVAL
    assert _list(lib, count=None, limit=0) == EINVAL
    assert _list(lib, ws=None) == EINVAL
    for field in ("key", "len", "value", "answered"):
        assert _list(lib, **{field: None}) == EINVAL, field
        assert _list(lib, limit=1, **{field: None}) == EINVAL, field
    assert _list(lib, limit=65) == EINVAL
    assert _list(lib, limit=2 ** 32 - 1) == EINVAL
    # flags: unknown bits, both bits of a pair, membership and `other` go together
    assert _list(lib, flags=NOT_IN_OTHER | 0x10) == EINVAL
    assert _list(lib, flags=0x80000000 | IN_OTHER) == EINVAL
    assert _list(lib, flags=IN_OTHER | NOT_IN_OTHER) == EINVAL
    assert _list(lib, flags=NOT_IN_OTHER | ANSWERED | UNANSWERED) == EINVAL
    assert _list(lib, other=None, flags=ANSWERED | UNANSWERED) == EINVAL
    assert _list(lib, other=None, flags=IN_OTHER) == EINVAL
    assert _list(lib, other=None, flags=NOT_IN_OTHER) == EINVAL
    assert _list(lib, flags=0) == EINVAL
    assert _list(lib, flags=ANSWERED) == EINVAL
    assert _list(lib, other=TABLE) == EINVAL
    assert _list(lib, other=TABLE, flags=IN_OTHER) == EINVAL
    # alignment
    assert _list(lib, table=TABLE + 32) == EINVAL
    assert _list(lib, other=OTHER + 8) == EINVAL
    assert _list(lib, count=0x100004) == EINVAL
    assert _list(lib, len=0x120002) == EINVAL
    assert _list(lib, value=0x130004) == EINVAL
    # workspace
    for limit in (0, 1, 10, 64):
        need = lib.sbe_inflight_list_workspace_size(limit)
        assert _list(lib, limit=limit, ws_bytes=need - 1) == ENOSPC
        assert _list(lib, limit=limit, other=None, flags=0, ws_bytes=need - 1) == ENOSPC
    assert _list(lib, ws_bytes=0) == ENOSPC


def test_log_init_refuses_bad_arguments(lib):
    need = lib.sbe_latency_log_size(8)
    assert need == 64 + 128
    assert lib.sbe_latency_log_init(None, need, 8, None) == EINVAL
    assert lib.sbe_latency_log_init(LOG + 32, need, 8, None) == EINVAL
    assert lib.sbe_latency_log_init(LOG, need - 1, 8, None) == EINVAL
    assert lib.sbe_latency_log_init(LOG, 1 << 40, 0, None) == EINVAL
    assert lib.sbe_latency_log_init(LOG, 1 << 40, 2 ** 31 + 1, None) == EINVAL


def _append(lib, log=LOG, code=CODE, value=VALUE, n=4, now=10, unit=1_000_000, tag=0, ws=WS, ws_bytes=1 << 20):
    return lib.sbe_latency_append(log, code, value, n, now, unit, tag, ws, ws_bytes, None)


def test_append_refuses_bad_arguments(lib):
    for name in ("log", "code", "value", "ws"):
        assert _append(lib, **{name: None}) == EINVAL, name
    assert _append(lib, log=LOG + 32) == EINVAL
    assert _append(lib, value=VALUE + 4) == EINVAL
    assert _append(lib, ws=WS + 4) == EINVAL
    assert _append(lib, n=2 ** 32) == EINVAL
    assert _append(lib, unit=0) == EINVAL
    assert _append(lib, unit=2 ** 62 + 1) == EINVAL
    assert _append(lib, unit=2 ** 63) == EINVAL
    for n in (1, 2048, 2049, 70000):
        assert _append(lib, n=n, ws_bytes=lib.sbe_latency_append_workspace_size(n) - 1) == ENOSPC
    assert _append(lib, ws_bytes=8) == ENOSPC
    # n == 0: only log is looked at, nothing is launched
    assert _append(lib, n=0, code=None, value=None, ws=None, ws_bytes=0, unit=0) == 0
    assert _append(lib, n=0, log=None) == EINVAL
    assert _append(lib, n=0, log=LOG + 8) == EINVAL


def _report(lib, log=LOG, pct=PCT7, n_pct=None, out="good", ws=WS, ws_bytes=1 << 20, **kw):
    o = ReportOut(*(0x200000 + 0x10000 * i for i in range(len(REPORT_OUT))))
    for k, v in kw.items():
        setattr(o, k, v)
    arr = None if pct is None else (ctypes.c_double * max(len(pct), 1))(*pct)
    n = (0 if pct is None else len(pct)) if n_pct is None else n_pct
    return lib.sbe_latency_report(log, arr, n, ctypes.byref(o) if out else None, ws, ws_bytes, None)


def test_report_refuses_bad_arguments(lib):
    assert _report(lib, log=None) == EINVAL
    assert _report(lib, out=None) == EINVAL
    assert _report(lib, count=None) == EINVAL
    assert _report(lib, stats=None) == EINVAL
    assert _report(lib, ws=None) == EINVAL
    assert _report(lib, pct=(50.0,) * 17) == EINVAL
    assert _report(lib, pct=None, n_pct=3) == EINVAL
    assert _report(lib, pct_value=None) == EINVAL
    assert _report(lib, pct_index=None) == EINVAL
    for bad in (float("nan"), float("inf"), -float("inf"), -1e-9, 100.00000001, 1e300):
        assert _report(lib, pct=(50.0, bad)) == EINVAL, bad
        assert _report(lib, pct=(bad,)) == EINVAL, bad
    assert _report(lib, log=LOG + 16) == EINVAL
    for i, field in enumerate(REPORT_OUT):
        assert _report(lib, **{field: 0x200000 + 0x10000 * i + (2 if field == "order" else 4)}) == EINVAL, field
    assert _report(lib, ws_bytes=lib.sbe_latency_report_workspace_size(1) - 1) == ENOSPC
    assert _report(lib, pct=(), ws_bytes=0) == ENOSPC
    assert _report(lib, count=None, stats=None, ws_bytes=0) == EINVAL  # arguments before the workspace
