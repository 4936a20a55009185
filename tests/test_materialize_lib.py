"""The MATERIALIZE case generator (tests/materialize_lib.py) on the CPU: every generated view lies
inside its record, the round model reproduces the hand-computed cases of the window / direct
boundary, and the families hold the classes the GPU tests (tests/test_gpu_materialize_edges.py) are
meant to reach.  The counts are conditions on the inputs, not measurements."""
import functools
import os
import re

import numpy as np
import pytest

import materialize_lib as M
import sbe_testlib as T


@functools.lru_cache(maxsize=None)
def fam(name):
    return {"W": M.family_w, "S": M.family_s}[name]()


def check_batch(b):
    n = b.n
    assert n % M.TILE == 0 or not b.names
    rl = (b.rec_off[1:] - b.rec_off[:-1]).astype(np.int64)
    assert (rl >= 1).all() and int(b.rec_off[-1]) == b.data.size
    end = b.view_off.astype(np.int64) + b.view_len.astype(np.int64)
    bad = np.nonzero((end > rl[:, None]).any(axis=1))[0]
    assert bad.size == 0, f"views outside their record at records {bad[:8]}"
    assert b.exp.size == int(b.view_len.sum(dtype=np.int64)) == int(b.exp_off[-1])
    assert ((b.data >= 32) & (b.data < 127)).all()


def test_constants_mirror_the_kernel():
    src = open(os.path.join(T.PKG, "csrc", "sbe_codec.hip")).read()
    assert int(re.search(r"#define SBE_MAT_WIN (\d+)", src).group(1)) == M.K_MAT_WIN
    assert re.search(r"fit - o > \(uint64_t\)\(kMatWin - 16\)", src) and M.DIRECT_OVER == M.K_MAT_WIN - 16
    assert re.search(r"kMatBlk = 1024;", src) and re.search(r"kMatTile = kWave;", src)
    assert M.SCAN_ROUND == 1024 * 1024 and M.TILE == 64
    assert all(n > M.SCAN_ROUND for n in M.N_SIZES)


# view bytes of the tile's records -> bytes a round loop that ignores direct records stores over
# them, with the span's start 0 / 1 / 15 bytes off 16-byte alignment (hand-computed)
MODEL_CASES = [
    ((1, 16370, 1), 16370, 16370, 0),
    ((7, 16369, 8), 16369, 0, 0),
    ((1, 16382, 1), 16382, 0, 0),
    ((1, 0, 16370, 0, 5), 16370, None, None),
    ((3, 16368, 3), 0, None, None),   # staged, not direct
    ((8, 16369, 8), 0, None, None),   # the span is longer than a window
    ((1, 16383, 1), 0, None, None),
    ((16370, 1), 0, None, None),
    ((1, 16370), 0, None, None),
]


@pytest.mark.parametrize("lens,w0,w1,w15", MODEL_CASES)
def test_round_model_on_hand_computed_tiles(lens, w0, w1, w15):
    for shift, want in ((0, w0), (1, w1), (15, w15)):
        if want is None:
            continue
        cls, clob = M.lens_classes(lens, 0, shift)
        assert clob == want, (lens, shift, clob)
        assert ("direct_between" in cls) == (want > 0)
        assert ("has_direct" in cls) == any(x > M.DIRECT_OVER for x in lens)


def test_bounded_rounds_stop_at_direct_records():
    """The rounds of a loop that ends at the next direct record never span one, and still finish
    every staged record, the record at each round's start first."""
    for lens in [c[0] for c in MODEL_CASES] + [(1, 16370, 1, 16370, 2), (5000,) * 9, (2, 2, 2, 16369, 1)]:
        for base in (0, 35):
            for shift in M.SHIFTS:
                o = list(base + np.concatenate([[0], np.cumsum(lens)[:-1]]))
                fit = list(base + np.cumsum(lens))
                direct = [i for i, x in enumerate(lens) if x > M.DIRECT_OVER]
                seen = []
                for start, cend, staged in M.rounds(o, fit, shift, bounded=True):
                    assert o[staged[0]] == start and cend - (start - ((shift + start) & 15)) <= M.K_MAT_WIN
                    assert all(not (o[i] < cend and fit[i] > start) for i in direct)
                    seen += staged
                assert sorted(seen) == [i for i, x in enumerate(lens) if 0 < x <= M.DIRECT_OVER]


def test_family_w():
    b = fam("W")
    check_batch(b)
    assert 900 <= b.tiles <= 2000 and b.data.size < 64 << 20
    for B in M.W_B:
        for lanes in M.W_LANES:
            for form in ("", "/5v"):  # B as one view and as five
                assert any(f" B={B}{form} c=" in s and f"lanes={lanes}" in s for s in b.names), (B, form, lanes)
    cl = M.classes(b, 0)
    between = [t for t, (c, _, _) in enumerate(cl) if "direct_between" in c]
    assert len(between) >= 50
    assert sum(1 for t in between if M.span_misalignment(b, t) != 0) >= 10
    assert sum(1 for c, _, _ in cl if "has_direct" in c and "direct_between" not in c) >= 20
    assert sum(1 for c, _, _ in cl if "has_direct" not in c) >= 20  # B at or under 16368: staged
    # the tiles placed at a chosen offset: the class follows the stated condition (the staged bytes of
    # the span plus its start's misalignment at most what the window has left beside the long record)
    placed = 0
    for t, s in enumerate(b.names):
        m = re.match(r"W at (\d+) mod 16: a=(\d+) B=(\d+) c=(\d+)", s)
        if m:
            r, a, B, c = map(int, m.groups())
            assert cl[t][2] % 16 == r
            assert ("direct_between" in cl[t][0]) == (a + c + r <= M.K_MAT_WIN - B), s
            placed += 1
    assert placed == 80
    for shift in M.SHIFTS:  # the class depends on the arena's address: enough such tiles at every shift run
        n = sum(1 for c, _, _ in M.classes(b, shift) if "direct_between" in c)
        assert n >= 20, (shift, n)


def test_family_s():
    b = fam("S")
    check_batch(b)
    rl = (b.rec_off[1:] - b.rec_off[:-1]).astype(np.int64)
    vo, vl = b.view_off.astype(np.int64), b.view_len.astype(np.int64)
    small = rl <= 40
    # every (record length, offset, length 0..15) occurs, the views ending at the record's end among them
    have = set()
    for k in range(5):
        have |= set(zip(rl[small].tolist(), vo[small, k].tolist(), vl[small, k].tolist()))
    want = {(r, o, ln) for r in range(1, 41) for o in range(r + 1) for ln in range(0, min(15, r - o) + 1)}
    assert want <= have
    live = vl > 0
    dec = ((np.diff(vo, axis=1) <= 0) | ~live[:, 1:] | ~live[:, :-1]).all(axis=1) & (live.sum(axis=1) >= 3)
    assert dec.sum() >= 300  # views in non-increasing source order
    lo, hi = vo[:, :, None], (vo + vl)[:, :, None]
    ov = (lo < hi.transpose(0, 2, 1)) & (lo.transpose(0, 2, 1) < hi) & live[:, :, None] & live[:, None, :]
    assert (ov.sum(axis=(1, 2)) > live.sum(axis=1)).sum() >= 300  # overlapping views
    mixed = ((vl >= 16) & (vl <= 48)).any(axis=1) & ((vl > 0) & (vl < 16)).any(axis=1)
    assert mixed.sum() >= 300
    at = b.exp_off[:-1:5].astype(np.int64)
    nonempty = vl.sum(axis=1) > 0
    assert np.bincount(at[nonempty] & 15, minlength=16).min() >= 100  # every arena alignment of a record
    assert np.bincount(np.arange(b.n)[nonempty] % M.TILE, minlength=M.TILE).min() >= 40  # every lane
    cl = M.classes(b, 0)
    assert sum(1 for c, _, _ in cl if "spans_two_rounds" in c) >= 20
    assert not any("has_direct" in c for c, _, _ in cl)


def test_family_c():
    cases = M.family_c()
    full_over_cut_under = cut_still_direct = 0
    for b, i, caps in cases:
        check_batch(b)
        at = b.exp_off[5 * i: 5 * i + 6].astype(np.int64).tolist()
        assert 0 in caps and at[5] - 1 in caps and at[5] in caps and at[5] + 1 in caps
        assert any(at[0] < c < at[0] + max(b.view_len[i]) for c in caps)
        assert any(at[5] < c < int(b.exp_off[-1]) for c in caps)       # inside c
        if (b.view_len[i] > 0).sum() == 5:
            assert set(at[1:5]) <= set(caps)
        for c in caps:
            o, fit = M.written(at, c)
            if fit < at[5] and at[5] - o > M.DIRECT_OVER:
                full_over_cut_under += 0 < fit - o <= M.DIRECT_OVER
                cut_still_direct += fit - o > M.DIRECT_OVER
    assert full_over_cut_under >= 2 and cut_still_direct >= 2


def test_family_n_small():
    """The generator of family N at a small n (the full sizes run in the GPU test)."""
    b = M.family_n(1000)
    check_batch(b)
    assert (b.view_len.sum(axis=1) == np.arange(1000) % 5).all()
    assert ((b.view_len > 0).sum(axis=0) > 100).all()  # every slot
