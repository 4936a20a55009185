"""What sbe_term_poll must give, composed from the two restatements the project holds
(termscan_lib.walk for the fragments, sbe_testlib.oracle_reassemble for the messages), and the
blocks the GPU test and the host program of tests/termpoll share."""
import numpy as np

import sbe_testlib as T
import termscan_lib as S

CARRY_LENGTHS = (1, 15, 16, 17, 1376, 70000)


def expect(block, start=0, limit=None, carry=b""):
    """counts (six), messages (list of bytes) and the carry out of a poll of block[start:] with at
    most `limit` fragments after an open accumulator `carry`."""
    w = S.walk(block, start, limit)
    c = len(carry)
    data = np.frombuffer(bytes(carry) + w["payload"], np.uint8)
    if c:
        off = np.array([0] + [c + x for x in w["frag_off"]], np.uint64)
        flags = np.array([0] + w["flags"], np.uint8)
    else:
        off = np.array(w["frag_off"], np.uint64)
        flags = np.array(w["flags"], np.uint8)
    msgs, carry_out = T.oracle_reassemble(data, off, flags)
    counts = [w["fragments"], w["next"], len(w["payload"]), w["stop"], len(msgs), len(carry_out)]
    return dict(counts=counts, msgs=msgs, carry=carry_out, walk=w)


def carry_bytes(n, seed=7):
    return np.random.default_rng(seed + n).integers(0, 256, n, dtype=np.uint8).tobytes()


def pattern(n, k):
    return bytes((k + 3 * j + (j >> 8)) & 0xff for j in range(n))


def edge_group_block(lead):
    """`lead` singles, then a BEGIN, thirty singles and the END: with lead = 1000 the group lies
    across fragment 1024 (the edge of a scan block) with singles inside on both sides."""
    b = S.Block()
    for k in range(lead):
        b.frame(pattern(1 + k % 5, k), 0xC0)
    b.frame(pattern(200, 1), 0x80)
    for k in range(30):
        b.frame(pattern(3 + k, k), 0xC0)
        if k % 4 == 0:
            b.frame(pattern(40 + k, 9 * k), 0x00)
    b.frame(pattern(77, 5), 0x40)
    b.frame(pattern(12, 6), 0xC0)
    return b.bytes()


def long_block(tile, single_inside=False, total=200000, mtu=1376):
    """One message of `total` bytes in frames of `mtu` payload bytes, small singles before and after,
    a padding frame in its middle; placed so that it crosses two tile edges (the first frame starts
    a little before an edge)."""
    b = S.Block()
    b.frame(b"before", 0xC0)
    b.frame(b"", 0xC0)
    b.pad_to(tile - 4 * 32)
    msg = pattern(total, 11)
    parts = [msg[k: k + mtu] for k in range(0, total, mtu)]
    for t, p in enumerate(parts):
        if t == len(parts) // 2:
            b.pad(96)
        if single_inside and t == 5:
            b.frame(b"a single inside the group", 0xC0)
        b.frame(p, (0x80 if t == 0 else 0) | (0x40 if t == len(parts) - 1 else 0))
    b.frame(b"after", 0xC0)
    b.frame(b"x" * 33, 0xC0)
    return b.bytes()


def open_limit(total=200000, mtu=1376, prefix=100000):
    """(limit, message bytes delivered to the accumulator) for long_block(single_inside=False)
    limited so that the message stays open with at least `prefix` bytes: two singles, then frames."""
    k = -(-prefix // mtu)
    return 2 + k, k * mtu


def carry_first_blocks():
    """(name, block, start, limit) for every first fragment a carry can meet."""
    out = []
    b = S.Block()
    b.frame(pattern(50, 1), 0x80)
    b.frame(pattern(60, 2), 0x40)
    b.frame(pattern(9, 3), 0xC0)
    out.append(("begin", b.bytes(), 0, None))
    b = S.Block()
    b.frame(pattern(70, 4), 0xC0)
    b.pad(64)
    b.frame(pattern(5, 5), 0xC0)
    out.append(("single", b.bytes(), 0, None))
    b = S.Block()
    b.frame(pattern(1376, 6), 0x00)
    b.frame(pattern(33, 7), 0x40)
    b.frame(pattern(8, 8), 0x80)
    out.append(("middle-end", b.bytes(), 0, None))
    b = S.Block()
    b.frame(pattern(31, 9), 0x40)
    b.frame(pattern(2, 10), 0xC0)
    out.append(("end", b.bytes(), 0, None))
    blk = out[0][1]
    out.append(("start-at-end", blk, len(blk), None))
    out.append(("limit-0", blk, 0, 0))
    out.append(("uncommitted", bytes(128), 0, None))
    return out


def host_cases(tile=32768):
    """The case list of the host program: termscan_lib.adversarial_cases() plus the long-message,
    edge-group and carry blocks of the GPU test, as (block, start, limit)."""
    cases = S.adversarial_cases(tile)
    lb = long_block(tile)
    cases += [(lb, 0, None), (long_block(tile, True), 0, None), (lb, 0, open_limit()[0])]
    cases += [(edge_group_block(1000), 0, None), (edge_group_block(999), 0, None)]
    cases += [(blk, start, limit) for _, blk, start, limit in carry_first_blocks()]
    return cases
