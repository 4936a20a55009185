"""CPU: the C ABI of sbe_json_extract_batch: the symbols, the header's constants, and argument
checks that return before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import jsonpaths_lib as J
import sbe_testlib as T
from test_jsonpaths_ref import BAD_TABLES, GOOD_TABLES

HEADER = os.path.join(T.ROOT, "include", "sbecodec.h")
EINVAL = -1
IN, REC, SEL, DOC, ROOT, KIND, OFF, LEN = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000


class Decoded(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("status", "flags", "hdr", "ts", "view_off", "view_len", "seq")]


class JsonPaths(ctypes.Structure):
    _fields_ = [("n_paths", ctypes.c_uint32), ("depth", ctypes.c_void_p), ("names", ctypes.c_void_p),
                ("name_off", ctypes.c_void_p)]


class JsonOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("doc", "root_kind", "kind", "off", "len")]


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(os.path.join(T.PKG, "libsbecodec.so"))
    vp = ctypes.c_void_p
    L.sbe_json_extract_workspace_size.restype = ctypes.c_size_t
    L.sbe_json_extract_workspace_size.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    L.sbe_json_extract_batch.restype = ctypes.c_int
    L.sbe_json_extract_batch.argtypes = [vp, vp, ctypes.c_uint64, ctypes.POINTER(Decoded), ctypes.c_uint32, vp,
                                         ctypes.POINTER(JsonPaths), ctypes.POINTER(JsonOut), vp, ctypes.c_size_t, vp]
    return L


def test_header_declares_and_library_exports(lib):
    text = open(HEADER).read()
    for name in ("sbe_json_extract_workspace_size", "sbe_json_extract_batch"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name)
    assert "sbe_json_extract_batch()" in text[: text.index("#ifndef SBECODEC_H")]
    assert "typedef struct sbe_json_paths" in text and "typedef struct sbe_json_out" in text
    names = "OK|NOT_SELECTED|EMPTY|FAILED|STACK"
    assert [int(v) for v in re.findall(r"#define SBE_JX_(?:%s) (\d+)u" % names, text)] == [0, 1, 2, 3, 4]
    kinds = re.findall(r"#define SBE_JX_(MISSING|STRING|STRING_ESC|NUMBER|TRUE|FALSE|NULL|OBJECT|ARRAY) (\d+)u", text)
    assert [int(v) for _, v in kinds] == list(range(9))
    topic = dict(re.findall(r"#define SBE_TOPIC_KIND_([A-Z_]+) (\d+)u", text))  # the kinds coincide where both exist
    assert all(topic[k] == v for k, v in kinds if k in topic) and len(topic) == 7
    caps = dict(re.findall(r"#define SBE_JSON_(MAX_PATHS|MAX_DEPTH|MAX_NAME|NAME_BYTES) (\d+)u", text))
    assert caps == {"MAX_PATHS": "16", "MAX_DEPTH": "4", "MAX_NAME": "64", "NAME_BYTES": "1024"}
    lib.sbe_abi_version.restype = ctypes.c_int
    assert lib.sbe_abi_version() == 8


def test_no_workspace(lib):
    for n, p in ((0, 1), (1, 16), (10 ** 6, 9), (2 ** 40, 16)):
        assert lib.sbe_json_extract_workspace_size(n, p) == 0


def _call(lib, table=("a.b", "s"), data=IN, rec=REC, n=4, dec=None, view=None, select=None, paths=True, out=True, **kw):
    P, depth, names, name_off = J.path_table(table)
    ps = JsonPaths(P, depth.ctypes.data, names.ctypes.data, name_off.ctypes.data)
    d = Decoded(0x90000, 0xA0000, 0xB0000, 0xC0000, 0xD0000, 0xE0000, None)
    o = JsonOut(DOC, ROOT, KIND, OFF, LEN)
    for k, v in kw.items():
        setattr(ps if hasattr(ps, k) else d if hasattr(d, k) else o, k, v)
    if view is None:
        view = 3 if dec else 0
    return lib.sbe_json_extract_batch(data, rec, n, ctypes.byref(d) if dec else None, view, select,
                                      ctypes.byref(ps) if paths else None, ctypes.byref(o) if out else None, None, 0, None)


def test_refuses_bad_arguments(lib):
    """The device pointers are never dereferenced here: every call is refused first."""
    assert _call(lib, data=None) == EINVAL
    assert _call(lib, rec=None) == EINVAL
    assert _call(lib, paths=False) == EINVAL
    assert _call(lib, out=False) == EINVAL
    assert _call(lib, paths=False, n=0) == EINVAL
    assert _call(lib, out=False, n=0) == EINVAL
    for f in ("doc", "root_kind", "kind", "off", "len", "depth", "names", "name_off"):
        assert _call(lib, **{f: None}) == EINVAL, f
    assert _call(lib, rec=REC + 4) == EINVAL
    assert _call(lib, off=OFF + 2) == EINVAL
    assert _call(lib, len=LEN + 1) == EINVAL
    assert _call(lib, n=2 ** 38) == EINVAL  # more 64-record tiles than a grid holds
    # the view goes with dec
    for view in (1, 2, 3, 4, 5):
        assert _call(lib, view=view) == EINVAL, view
    for view in (0, 1, 2, 5, 2 ** 31):
        assert _call(lib, dec=True, view=view) == EINVAL, view
    assert _call(lib, dec=True, view=4, n=0) == 0
    for f in ("status", "flags", "view_off", "view_len"):
        assert _call(lib, dec=True, **{f: None}) == EINVAL, f
    assert _call(lib, dec=True, view_off=0xD0002) == EINVAL
    assert _call(lib, dec=True, view_len=0xE0001) == EINVAL
    assert _call(lib, n_paths=0) == EINVAL
    assert _call(lib, n_paths=17) == EINVAL


def test_empty_batch_launches_nothing(lib):
    assert _call(lib, n=0) == 0
    assert _call(lib, n=0, data=None, rec=None, doc=None, kind=None) == 0  # only the table and the view are looked at
    assert _call(lib, n=0, select=SEL) == 0


@pytest.mark.parametrize("table,what", BAD_TABLES[1:], ids=[w for _, w in BAD_TABLES[1:]])
def test_refuses_bad_path_tables(lib, table, what):
    assert _call(lib, table=table) == EINVAL
    assert _call(lib, table=table, n=0) == EINVAL


def test_accepts_good_path_tables(lib):
    for table in GOOD_TABLES:
        assert _call(lib, table=table, n=0) == 0, table


def test_name_offsets_must_rise(lib):
    two = ("abcdefgh", "s")  # two names in a buffer of ten bytes
    off = np.array([0, 1, 1], np.uint32)  # the second name is empty
    assert _call(lib, table=two, name_off=off.ctypes.data) == EINVAL
    off = np.array([0, 2, 1], np.uint32)
    assert _call(lib, table=two, name_off=off.ctypes.data) == EINVAL
    off = np.array([5, 6, 7], np.uint32)  # need not start at 0
    assert _call(lib, table=two, name_off=off.ctypes.data, n=0) == 0
    off = np.array([5, 6, 6 + 65], np.uint32)  # refused before the name is read
    assert _call(lib, table=two, name_off=off.ctypes.data) == EINVAL
