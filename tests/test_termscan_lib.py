"""CPU: the Python restatement of the term-buffer walk (tests/termscan_lib.py) against the hand
cases, whose expected tables are written out, and the properties of the shared blocks the GPU tests
lean on (the tile block does put frames where its comments say)."""
import pytest

import termscan_lib as S


@pytest.mark.parametrize("case", S.HAND_CASES, ids=[c[0] for c in S.HAND_CASES])
def test_hand_cases(case):
    _, blk, start, limit, exp = case
    got = S.walk(blk, start, limit)
    for k, v in exp.items():
        assert got[k] == v, k
    assert len(got["payload"]) == got["frag_off"][-1]


def test_decoys_never_surface():
    blk, real = S.decoy_block()
    w = S.walk(blk)
    assert w["frag_src"] == real and w["stop"] == S.END and w["next"] == len(blk)
    assert S.walk(blk, 0, 5)["frag_src"] == real[:5]


def test_tile_block_touches_the_edges():
    t = 4096
    blk = S.tile_block(t)
    w = S.walk(blk)
    src = w["frag_src"]
    ends = [s + S.align(32 + n) for s, n in zip(src, [b - a for a, b in zip(w["frag_off"], w["frag_off"][1:])])]
    assert t in ends                                                  # a frame ends exactly at the first edge
    assert any(s < 2 * t < e for s, e in zip(src, ends))              # one straddles the second
    assert 7 * t - 32 in src and 8 * t - 32 in src                    # frames in the last slot of a tile
    assert not any(3 * t <= s < 6 * t for s in src)                   # three whole tiles under one padding frame
    assert w["stop"] == S.END and w["next"] == len(blk)


def test_stop_blocks():
    for name, blk in S.stop_blocks(4096):
        w = S.walk(blk)
        want = {"short": S.SHORT, "partial": S.PARTIAL, "partial-max": S.PARTIAL, "uncommitted": S.UNCOMMITTED,
                "negative": S.UNCOMMITTED}[name.rsplit("-", 1)[0]]
        assert w["stop"] == want, name
        assert w["next"] == len(blk) - 32 * 4 - 64 and w["fragments"] == (1 if name.endswith("first") else 3), name


def test_dense_blocks_have_long_chains_in_a_tile():
    t = 32768
    for name, blk in S.dense_blocks(t):
        assert len(blk) > 3 * t, name
        # frames consumed inside each whole tile: more than the 512 steps one doubling level reaches
        offset, per_tile = 0, [0, 0, 0]
        while offset < 3 * t:
            per_tile[offset // t] += 1
            offset += S.align(int.from_bytes(blk[offset: offset + 4], "little"))
        assert min(per_tile) > 512 + 128, (name, per_tile)
        w = S.walk(blk)
        assert w["stop"] == S.END and w["next"] == len(blk), name
    assert S.walk(S.dense_blocks(t)[0][1])["fragments"] == 3 * 1024 + 37
    assert S.walk(S.dense_blocks(t)[1][1])["fragments"] == 0


def test_random_block_is_full_and_mixed():
    blk = S.random_block(4096, 11)
    w = S.walk(blk)
    assert len(blk) == 32 * 4096 and w["stop"] == S.END and w["next"] == len(blk) and w["fragments"] > 100
