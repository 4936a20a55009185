"""MATERIALIZE (sbe_materialize_views) at the edges of its copy kernel, on hand-built descriptors
(tests/materialize_lib.py) against the plain gather sbe_testlib.oracle_materialize, bit-exact:

  W  records around the window / direct-copy boundary, between small records of the same tile
  S  views under 16 bytes at every offset of records of 1..40 bytes, unordered and overlapping
  C  capacities that cut a long record's views, with the arena untouched from the last view written
  N  more records than one round of the block-sum scan takes
  and the call contract: alignment checks before any launch, status required but never read.

Every batch runs with the arena tensor advanced by 0, 1, 8 and 15 bytes."""
import ctypes
import functools

import numpy as np
import pytest

import materialize_lib as M

pytestmark = pytest.mark.gpu

SLACK = 4096
FILL = 0xA5
SBE_EINVAL = -1


@functools.lru_cache(maxsize=None)
def family(name):
    return {"W": M.family_w, "S": M.family_s}[name]()


class DevBatch:
    """A Batch's inputs on the device, the descriptors passed through codec.Decoded."""

    def __init__(self, codec, b, status_fill=0):
        import torch
        self.b = b
        self.data = torch.from_numpy(b.data).cuda()
        self.rec_off = torch.from_numpy(b.rec_off.view(np.int64)).cuda()
        n = b.n
        self.dec = codec.Decoded(torch.full((n,), status_fill, dtype=torch.uint8, device="cuda"),
                                 torch.zeros(n, dtype=torch.uint8, device="cuda"),
                                 torch.zeros((n, 4), dtype=torch.int16, device="cuda"),
                                 torch.zeros(n, dtype=torch.int64, device="cuda"),
                                 torch.from_numpy(b.view_off.view(np.int32)).cuda(),
                                 torch.from_numpy(b.view_len.view(np.int32)).cuda())

    def run(self, codec, shift=0, cap=None):
        """(buf, arena_off): buf is the whole allocation (shift bytes, the arena, the slack), filled
        with FILL before the call; the arena starts at buf[shift]."""
        import torch
        total = int(self.b.exp_off[-1])
        buf = torch.full((shift + total + SLACK,), FILL, dtype=torch.uint8, device="cuda")
        arena = buf[shift:]
        assert arena.data_ptr() % 16 == shift
        m = codec.materialize_views(self.data, self.rec_off, self.dec, arena=arena,
                                    arena_capacity=total if cap is None else cap)
        torch.cuda.synchronize()
        return buf.cpu().numpy(), m.arena_off.cpu().numpy().view(np.uint64)


def tile_report(b, got, shift, cap=None):
    """None, or which tiles hold wrong arena bytes: name, classes, first wrong arena offset."""
    bad = np.nonzero(got[: b.exp.size] != b.exp)[0]
    if bad.size == 0:
        return None
    cl = M.classes(b, shift, cap)
    starts = np.array([c[2] for c in cl], np.int64)
    tiles = np.searchsorted(starts, bad, side="right") - 1
    lines, by_class = [], {}
    for t in np.unique(tiles):
        first = int(bad[tiles == t][0])
        key = ",".join(sorted(cl[t][0])) or "none"
        by_class[key] = by_class.get(key, 0) + 1
        if len(lines) < 12:
            lines.append(f"tile {t} [{b.names[t] if t < len(b.names) else ''}] classes {{{key}}}: "
                         f"{int((tiles == t).sum())} wrong bytes (model: {cl[t][1]}), first at arena offset {first} "
                         f"(tile offset {int(starts[t])})")
    between = {t for t, c in enumerate(cl) if "direct_between" in c[0]}
    return (f"shift {shift}: {bad.size} wrong arena bytes in {np.unique(tiles).size} tiles "
            f"({len(between & set(tiles.tolist()))} of the {len(between)} direct_between tiles), by class {by_class}\n"
            + "\n".join(lines))


def class_counts(b, shift):
    out = {}
    for c, _, _ in M.classes(b, shift):
        for k in c or {"none"}:
            out[k] = out.get(k, 0) + 1
    return out


@pytest.mark.parametrize("name", ["W", "S"])
def test_gpu_materialize_window_edges(codec, name):
    """Families W and S: arena_off and every arena byte equal the oracle's at each arena alignment;
    nothing before the arena or after the total is written."""
    b = family(name)
    dev = DevBatch(codec, b)
    total = b.exp.size
    failures = []
    for shift in M.SHIFTS:
        print(f"family {name} shift {shift}: {b.tiles} tiles, classes {class_counts(b, shift)}")
        buf, off = dev.run(codec, shift)
        assert np.array_equal(off, b.exp_off), f"shift {shift}: arena_off differs from the oracle"
        got = buf[shift:]
        msg = tile_report(b, got, shift)
        if msg:
            failures.append(msg)
        assert (buf[:shift] == FILL).all(), f"shift {shift}: bytes before the arena written"
        assert (got[total:] == FILL).all(), f"shift {shift}: bytes past the total written"
    assert not failures, "\n".join(failures)


def test_gpu_materialize_capacity_cuts(codec):
    """Family C: arena_off holds the full layout, every view that ends within the capacity is exact,
    and every byte from the end of the last view written on, through the slack, is untouched."""
    failures = []
    calls = 0
    for b, i, caps in M.family_c():
        dev = DevBatch(codec, b)
        ends = b.exp_off[1:].astype(np.int64)
        for cap in caps:
            shift = M.SHIFTS[calls % len(M.SHIFTS)]
            calls += 1
            buf, off = dev.run(codec, shift, cap)
            got = buf[shift:]
            what = f"[{b.names[-1]}] cap {cap} (B at {int(b.exp_off[5 * i])}..{int(b.exp_off[5 * i + 5])}) shift {shift}"
            assert np.array_equal(off, b.exp_off), what
            fit = ends <= cap
            last = int(ends[fit].max()) if fit.any() else 0
            # the views written are a prefix of the layout: exact up to the end of the last of them
            wrong = np.nonzero(got[:last] != b.exp[:last])[0]
            if wrong.size:
                failures.append(f"{what}: {wrong.size} wrong bytes below {last}, first at {int(wrong[0])}; "
                                f"classes {M.classes(b, shift, cap)[-1][0]}")
            stray = np.nonzero(got[last:] != FILL)[0]
            if stray.size:
                failures.append(f"{what}: {stray.size} bytes written from {last} on, first at {last + int(stray[0])}")
            assert (buf[:shift] == FILL).all(), what
    print(f"family C: {calls} calls")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n", M.N_SIZES)
def test_gpu_materialize_scan_carry(codec, n):
    """Family N: the block-sum scan's second loop round carries the first round's total."""
    b = M.family_n(n)
    assert n > M.SCAN_ROUND
    buf, off = DevBatch(codec, b).run(codec)
    assert int(off[5 * n]) == b.exp.size == int(b.view_len.sum(dtype=np.int64))
    bad = np.nonzero(off != b.exp_off)[0]
    assert bad.size == 0, f"arena_off differs from entry {bad[0]} (record {bad[0] // 5}) on"
    bad = np.nonzero(buf[: b.exp.size] != b.exp)[0]
    assert bad.size == 0, f"{bad.size} wrong arena bytes, first at {bad[0]}"
    assert (buf[b.exp.size:] == FILL).all()


# ------------------------------------------------------------------------------------------
# the call contract, through the C entry point
# ------------------------------------------------------------------------------------------
def raw_call(codec, data, rec_off, n, status, view_off, view_len, arena, cap, arena_off, ws):
    """sbe_materialize_views with raw addresses (ints), as a C caller would pass them."""
    import torch
    d = codec._Decoded(status, None, None, None, view_off, view_len, None)  # sbe_decoded: flags, hdr, ts, seq unused
    vp = ctypes.c_void_p
    return codec.lib().sbe_materialize_views(vp(data), vp(rec_off), n, ctypes.byref(d), vp(arena), cap, vp(arena_off),
                                             vp(ws.data_ptr()), int(ws.numel()),
                                             vp(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("which,by", [("rec_off", 4), ("arena_off", 4), ("view_off", 1), ("view_off", 2),
                                      ("view_len", 1), ("view_len", 2)])
def test_gpu_materialize_rejects_misaligned_arrays(codec, which, by):
    """rec_off / arena_off off 8-byte alignment, view_off / view_len off 4-byte alignment:
    SBE_EINVAL before any launch, arena and arena_off untouched.  The arrays are built so that the
    advanced pointer still reads what the aligned one does (every record at offset 0 of the input;
    all-zero descriptors where view_off / view_len move) and stays inside its allocation."""
    import torch
    n = 200
    data = torch.randint(32, 127, (256,), dtype=torch.uint8, device="cuda")
    rec_off = torch.zeros(n + 4, dtype=torch.int64, device="cuda")
    moved_views = which in ("view_off", "view_len")
    view_off = torch.zeros(5 * n + 4, dtype=torch.int32, device="cuda")
    view_len = torch.zeros(5 * n + 4, dtype=torch.int32, device="cuda")
    if not moved_views:
        view_off[: 5 * n] = torch.arange(5 * n, dtype=torch.int32, device="cuda") % 97
        view_len[: 5 * n] = torch.arange(5 * n, dtype=torch.int32, device="cuda") % 23
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    total = int(view_len[: 5 * n].sum().item())
    arena = torch.full((total + SLACK,), FILL, dtype=torch.uint8, device="cuda")
    arena_off = torch.full((5 * n + 4,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
    ws = torch.zeros(int(codec.lib().sbe_materialize_workspace_size(n)) + 16, dtype=torch.uint8, device="cuda")
    ptr = {"rec_off": rec_off.data_ptr(), "arena_off": arena_off.data_ptr(), "view_off": view_off.data_ptr(),
           "view_len": view_len.data_ptr()}
    before = arena_off.clone()

    def call():
        rc = raw_call(codec, data.data_ptr(), ptr["rec_off"], n, status.data_ptr(), ptr["view_off"], ptr["view_len"],
                      arena.data_ptr(), total, ptr["arena_off"], ws)
        torch.cuda.synchronize()
        return rc

    ptr[which] += by
    assert call() == SBE_EINVAL
    assert bool((arena == FILL).all()) and torch.equal(arena_off, before)
    ptr[which] -= by  # the same call with the array where it belongs goes through
    assert call() == 0
    assert int(arena_off[5 * n]) == total and (moved_views or not bool((arena[:total] == FILL).all()))


def test_gpu_materialize_ignores_status(codec):
    """status must be there and is not read: all 0xFF gives what all zeros gives, the oracle's arena."""
    b = family("S")
    outs = []
    for fill in (0, 0xFF):
        buf, off = DevBatch(codec, b, status_fill=fill).run(codec, shift=8)
        assert np.array_equal(off, b.exp_off)
        outs.append(buf)
    assert np.array_equal(outs[0], outs[1])
    assert tile_report(b, outs[1][8:], 8) is None
