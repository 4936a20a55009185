"""CPU: the C ABI of the *_counted calls (record counts held in device memory): declarations and
exports, and every SBE_EINVAL / SBE_ENOSPC line of their contract returned before anything touches
a device (fake pointers, no device): whatever the base call refuses with n = n_capacity, a null or
misaligned n_dev with n_capacity > 0, a misaligned rec_idx, n_capacity past the base call's limit,
a bad argument ahead of a short workspace."""
import ctypes
import os
import re

import pytest

import sbe_testlib as T

HEADER = os.path.join(T.ROOT, "include", "sbecodec.h")
OK, EINVAL, ENOSPC = 0, -1, -3
NAMES = ("sbe_decode_batch_counted", "sbe_classify_commits_counted", "sbe_emit_commit_offsets_counted",
         "sbe_term_append_counted")
P = [0x100000 * k for k in range(1, 40)]  # fake device addresses, 1 MiB apart
vp, u64, u32, i64, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64, ctypes.c_size_t


class Decoded(ctypes.Structure):
    _fields_ = [(k, vp) for k in ("status", "flags", "hdr", "ts", "view_off", "view_len", "seq")]


class CommitOut(ctypes.Structure):
    _fields_ = [(k, vp) for k in ("cm", "topic_src", "topic_kind", "topic_off", "topic_len", "topic_idx", "last", "count")]


class EmitOut(ctypes.Structure):
    _fields_ = [(k, vp) for k in ("out_off", "status", "emit_idx", "totals")]


class Fallback(ctypes.Structure):
    _fields_ = [("topic_arena", vp), ("topic_off", vp), ("default_ident", vp), ("default_ident_len", u32), ("now_ns", u64),
                ("uuid_ns", u64)]


class TermHeader(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("session_id", "stream_id", "term_id", "term_offset_base")] + [("version", ctypes.c_uint8)]


class AppendOut(ctypes.Structure):
    _fields_ = [(k, vp) for k in ("rec_tail", "counts")]


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(os.path.join(T.PKG, "libsbecodec.so"))
    L.sbe_decode_batch_counted.argtypes = [vp, vp, vp, u64, u64, u32, ctypes.POINTER(Decoded), vp]
    L.sbe_classify_commits_counted.argtypes = [vp, vp, vp, u64, ctypes.POINTER(Decoded), vp, vp, u32,
                                               ctypes.POINTER(CommitOut), vp, sz, vp]
    L.sbe_emit_commit_offsets_counted.argtypes = [vp, vp, vp, u64, ctypes.POINTER(Decoded), ctypes.POINTER(CommitOut), vp, vp,
                                                  vp, u32, vp, u32, ctypes.c_int, i64, i64, vp, u64, ctypes.POINTER(EmitOut),
                                                  vp, sz, vp, ctypes.POINTER(Fallback)]
    L.sbe_term_append_counted.argtypes = [vp, u64, vp, vp, vp, u64, vp, u64, u64, u64, u32, u64, ctypes.POINTER(TermHeader),
                                          ctypes.POINTER(AppendOut), vp, sz, vp]
    for n in NAMES:
        getattr(L, n).restype = ctypes.c_int
    for n in ("sbe_commit_emit_workspace_size", "sbe_term_append_workspace_size"):
        getattr(L, n).restype = sz
        getattr(L, n).argtypes = [u64]
    L.sbe_abi_version.restype = ctypes.c_int
    return L


def test_header_declares_and_library_exports(lib):
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert hasattr(lib, name), name
    assert "n = min(*n_dev, n_capacity)" in text
    assert "#define SBECODEC_ABI_VERSION 8" in text and lib.sbe_abi_version() == 8


def test_python_binding_names_the_calls():
    src = open(os.path.join(T.PKG, "sbecodec.py")).read()
    for name in ("def decode_batch_counted(", "def classify_commits_counted(", "def emit_commit_offsets_counted(",
                 "def term_append_counted(", "def egress_commit_step("):
        assert name in src, name
    # the counted section reads nothing back from the device
    body = src[src.index("# ---- record counts held in device memory"): src.index("# bytes per order of the default output bound")]
    for word in (".item()", ".cpu()", ".tolist()", ".numpy()"):
        assert word not in body, word


# ---- sbe_decode_batch_counted ----
def _decode(lib, data=P[0], rec_off=P[1], n_dev=P[2], cap=100, avg=0, mode=0, out="good", **ptr):
    d = dict(status=P[3], flags=P[4], hdr=P[5], ts=P[6], view_off=P[7], view_len=P[8], seq=P[9])
    d.update(ptr)
    o = Decoded(*(d[k] for k, _ in Decoded._fields_))
    return lib.sbe_decode_batch_counted(data, rec_off, n_dev, cap, avg, mode, ctypes.byref(o) if out else None, None)


def test_decode_refuses_bad_arguments(lib):
    assert _decode(lib, n_dev=None) == EINVAL
    assert _decode(lib, n_dev=P[2] + 4) == EINVAL
    assert _decode(lib, mode=3) == EINVAL
    for name in ("data", "rec_off", "out"):
        assert _decode(lib, **{name: None}) == EINVAL, name
    for name in ("status", "flags", "hdr", "ts", "view_off", "view_len"):
        assert _decode(lib, **{name: None}) == EINVAL, name
    assert _decode(lib, data=P[0] + 8) == EINVAL
    assert _decode(lib, rec_off=P[1] + 4) == EINVAL
    assert _decode(lib, hdr=P[5] + 4) == EINVAL and _decode(lib, ts=P[6] + 4) == EINVAL
    assert _decode(lib, view_off=P[7] + 2) == EINVAL and _decode(lib, view_len=P[8] + 2) == EINVAL
    assert _decode(lib, seq=P[9] + 4) == EINVAL
    assert _decode(lib, cap=64 * 0xFFFFFFFF + 1) == EINVAL  # past the base call's limit on n
    # an empty capacity: nothing is launched, n_dev is not looked at
    assert _decode(lib, cap=0, n_dev=None) == OK and _decode(lib, cap=0, n_dev=P[2] + 4, data=None, rec_off=None) == OK
    assert _decode(lib, cap=0, mode=3) == EINVAL


# ---- sbe_classify_commits_counted ----
def _classify(lib, data=P[0], rec_off=P[1], n_dev=P[2], cap=100, dec="good", tarena=P[10], toff=P[11], k=3, out="good", **ptr):
    d = dict(status=P[3], flags=P[4], hdr=P[5], ts=P[6], view_off=P[7], view_len=P[8], seq=None,
             cm=P[12], topic_src=P[13], topic_kind=P[14], topic_off=P[15], topic_len=P[16], topic_idx=P[17], last=P[18], count=P[19])
    d.update(ptr)
    de = Decoded(*(d[f] for f, _ in Decoded._fields_))
    o = CommitOut(*(d[f] for f, _ in CommitOut._fields_))
    return lib.sbe_classify_commits_counted(data, rec_off, n_dev, cap, ctypes.byref(de) if dec else None, tarena, toff, k,
                                            ctypes.byref(o) if out else None, None, 0, None)


def test_classify_refuses_bad_arguments(lib):
    assert _classify(lib, n_dev=None) == EINVAL
    assert _classify(lib, n_dev=P[2] + 4) == EINVAL
    for cap in (0, 100):  # whatever the capacity
        assert _classify(lib, cap=cap, out=None) == EINVAL
        assert _classify(lib, cap=cap, last=None) == EINVAL and _classify(lib, cap=cap, count=None) == EINVAL
        assert _classify(lib, cap=cap, last=P[18] + 4) == EINVAL and _classify(lib, cap=cap, count=P[19] + 4) == EINVAL
        assert _classify(lib, cap=cap, k=0) == EINVAL and _classify(lib, cap=cap, k=65) == EINVAL
    for name in ("data", "rec_off", "dec", "tarena", "toff", "status", "flags", "view_off", "view_len", "cm", "topic_src",
                 "topic_kind", "topic_off", "topic_len", "topic_idx"):
        assert _classify(lib, **{name: None}) == EINVAL, name
    assert _classify(lib, rec_off=P[1] + 4) == EINVAL
    for name, at in (("view_off", 7), ("view_len", 8), ("topic_off", 15), ("topic_len", 16), ("topic_idx", 17)):
        assert _classify(lib, **{name: P[at] + 2}) == EINVAL, name
    assert _classify(lib, toff=P[11] + 2) == EINVAL
    assert _classify(lib, cap=64 * 0x7FFFFFFF + 1) == EINVAL


# ---- sbe_emit_commit_offsets_counted ----
def _emit(lib, data=P[0], rec_off=P[1], n_dev=P[2], cap=100, dec="good", plan="good", tid=P[20], iarena=P[21], ioff=P[22], k=3,
          mask=None, eflags=0, session=1, out=P[23], out_cap=1 << 16, res="good", ws=P[24], ws_bytes=None, fb=None, **ptr):
    d = dict(status=P[3], flags=P[4], hdr=P[5], ts=P[6], view_off=P[7], view_len=P[8], seq=P[9],
             cm=P[12], topic_src=P[13], topic_kind=P[14], topic_off=P[15], topic_len=P[16], topic_idx=P[17], last=P[18], count=P[19],
             out_off=P[25], est=P[26], emit_idx=P[27], totals=P[28])
    d.update(ptr)
    de = Decoded(*(d[f] for f, _ in Decoded._fields_))
    pl = CommitOut(*(d[f] for f, _ in CommitOut._fields_))
    r = EmitOut(d["out_off"], d["est"], d["emit_idx"], d["totals"])
    if ws_bytes is None:
        ws_bytes = lib.sbe_commit_emit_workspace_size(cap)
    f = None
    if fb:
        fd = dict(topic_arena=P[10], topic_off=P[11], default_ident=P[29], default_ident_len=8, now_ns=1, uuid_ns=2)
        fd.update(fb if isinstance(fb, dict) else {})
        f = ctypes.byref(Fallback(*(fd[x] for x, _ in Fallback._fields_)))
    return lib.sbe_emit_commit_offsets_counted(data, rec_off, n_dev, cap, ctypes.byref(de) if dec else None,
                                               ctypes.byref(pl) if plan else None, tid, iarena, ioff, k, mask, eflags, session, 3, 4,
                                               out, out_cap, ctypes.byref(r) if res else None, ws, ws_bytes, None, f)


def test_emit_refuses_bad_arguments(lib):
    for fb in (None, True):
        assert _emit(lib, fb=fb, n_dev=None) == EINVAL
        assert _emit(lib, fb=fb, n_dev=P[2] + 4) == EINVAL
        for cap in (0, 100):
            assert _emit(lib, fb=fb, cap=cap, res=None) == EINVAL
            assert _emit(lib, fb=fb, cap=cap, out_off=None) == EINVAL and _emit(lib, fb=fb, cap=cap, totals=None) == EINVAL
            assert _emit(lib, fb=fb, cap=cap, out_off=P[25] + 4) == EINVAL and _emit(lib, fb=fb, cap=cap, totals=P[28] + 4) == EINVAL
            assert _emit(lib, fb=fb, cap=cap, emit_idx=P[27] + 4) == EINVAL
            assert _emit(lib, fb=fb, cap=cap, k=0) == EINVAL and _emit(lib, fb=fb, cap=cap, k=65) == EINVAL
            assert _emit(lib, fb=fb, cap=cap, eflags=2) == EINVAL and _emit(lib, fb=fb, cap=cap, eflags=1, mask=P[30]) == EINVAL
            assert _emit(lib, fb=fb, cap=cap, session=2) == EINVAL
            assert _emit(lib, fb=fb, cap=cap, out=None) == EINVAL
        for name in ("data", "rec_off", "dec", "plan", "tid", "iarena", "ioff", "ws", "status", "flags", "view_off", "view_len", "cm",
                     "topic_idx", "est"):
            assert _emit(lib, fb=fb, **{name: None}) == EINVAL, name
        assert _emit(lib, fb=fb, eflags=1, last=None) == EINVAL
        assert _emit(lib, fb=fb, rec_off=P[1] + 4) == EINVAL and _emit(lib, fb=fb, seq=P[9] + 4) == EINVAL
        assert _emit(lib, fb=fb, tid=P[20] + 2) == EINVAL and _emit(lib, fb=fb, ioff=P[22] + 2) == EINVAL
        assert _emit(lib, fb=fb, ws=P[24] + 8) == EINVAL
        assert _emit(lib, fb=fb, cap=1 << 32) == EINVAL
    for bad in (dict(topic_arena=None), dict(topic_off=None), dict(default_ident=None), dict(topic_off=P[11] + 2),
                dict(default_ident_len=4097)):
        for cap in (0, 100):
            assert _emit(lib, fb=bad, cap=cap) == EINVAL, bad
    for name in ("ts", "topic_kind", "topic_off", "topic_len"):
        assert _emit(lib, fb=True, **{name: None}) == EINVAL, name
    assert _emit(lib, fb=True, ts=P[6] + 4) == EINVAL


def test_emit_short_workspace(lib):
    need = lib.sbe_commit_emit_workspace_size(100)
    assert _emit(lib, ws_bytes=need - 1) == ENOSPC and _emit(lib, ws_bytes=0, fb=True) == ENOSPC
    # the workspace is the capacity's, and a bad argument wins over a short one
    assert _emit(lib, cap=1 << 20, ws_bytes=lib.sbe_commit_emit_workspace_size(1 << 20) - 1) == ENOSPC
    assert _emit(lib, ws_bytes=0, n_dev=None) == EINVAL
    assert _emit(lib, ws_bytes=0, n_dev=P[2] + 4) == EINVAL
    assert _emit(lib, ws_bytes=0, k=0) == EINVAL


# ---- sbe_term_append_counted ----
def _append(lib, data=P[0], in_bytes=4096, rec_off=P[1], rec_idx=P[31], n_dev=P[2], cap=10, block=P[32], nbytes=4096, start=0,
            limit=(1 << 64) - 1, mtu=1408, max_len=1 << 20, hdr="good", o="good", ws=P[33], ws_bytes=None, rec_tail=P[34],
            counts=P[35]):
    h = TermHeader(1, 2, 3, 0, 1)
    out = AppendOut(rec_tail, counts)
    if ws_bytes is None:
        ws_bytes = lib.sbe_term_append_workspace_size(cap)
    return lib.sbe_term_append_counted(data, in_bytes, rec_off, rec_idx, n_dev, cap, block, nbytes, start, limit, mtu, max_len,
                                       ctypes.byref(h) if hdr else None, ctypes.byref(out) if o else None, ws, ws_bytes, None)


def test_append_refuses_bad_arguments(lib):
    assert _append(lib, n_dev=None) == EINVAL
    assert _append(lib, n_dev=P[2] + 4) == EINVAL
    for cap in (0, 10):
        assert _append(lib, cap=cap, rec_idx=P[31] + 4) == EINVAL
        assert _append(lib, cap=cap, hdr=None) == EINVAL and _append(lib, cap=cap, o=None) == EINVAL
        assert _append(lib, cap=cap, counts=None) == EINVAL
        assert _append(lib, cap=cap, nbytes=4096 + 16) == EINVAL and _append(lib, cap=cap, start=8) == EINVAL
        assert _append(lib, cap=cap, start=4096 + 32) == EINVAL and _append(lib, cap=cap, nbytes=(1 << 30) + 32) == EINVAL
        for mtu in (0, 32, 48, 1400, 65536):
            assert _append(lib, cap=cap, mtu=mtu) == EINVAL, mtu
        assert _append(lib, cap=cap, max_len=(1 << 30) + 1) == EINVAL
        assert _append(lib, cap=cap, block=P[32] + 8) == EINVAL and _append(lib, cap=cap, rec_off=P[1] + 4) == EINVAL
        assert _append(lib, cap=cap, rec_tail=P[34] + 4) == EINVAL and _append(lib, cap=cap, counts=P[35] + 4) == EINVAL
    for name in ("rec_off", "data", "block", "ws"):
        assert _append(lib, **{name: None}) == EINVAL, name
    assert _append(lib, cap=1 << 32) == EINVAL


def test_append_short_workspace(lib):
    need = lib.sbe_term_append_workspace_size(10)
    assert _append(lib, ws_bytes=need - 1) == ENOSPC and _append(lib, ws_bytes=0, rec_idx=None) == ENOSPC
    assert _append(lib, cap=1 << 20, ws_bytes=lib.sbe_term_append_workspace_size(1 << 20) - 1) == ENOSPC
    assert _append(lib, ws_bytes=0, n_dev=None) == EINVAL
    assert _append(lib, ws_bytes=0, n_dev=P[2] + 4) == EINVAL
    assert _append(lib, ws_bytes=0, rec_idx=P[31] + 4) == EINVAL
    assert _append(lib, ws_bytes=0, start=8) == EINVAL
