"""GPU: the host mirror's FragmentReassembler::on_term_block (tests/term/test_term_host.cpp) against
term_walk + on_fragments, over the tile-edge block of tests/termscan_lib.py (whole, limited and
restarted) and a message that spans two blocks, polled one after another by one reassembler."""
import os
import re
import subprocess

import pytest

import termscan_lib as S

pytestmark = pytest.mark.gpu


def test_on_term_block_against_walk_and_on_fragments(codec, tmp_path):
    t = codec.term_scan_tile()
    edge = S.tile_block(t)
    first = S.walk(edge, 0, 3)
    # a message of 5000 bytes in frames of 1376: BEGIN and one middle in the first block, the rest
    # in the second, between whole messages
    msg = bytes((11 * j) & 0xff for j in range(5000))
    a, b = S.Block(), S.Block()
    a.frame(b"whole-1", 0xC0)
    a.frame(msg[:1376], 0x80)
    a.frame(msg[1376:2752], 0x00)
    b.frame(msg[2752:4128], 0x00)
    b.pad(64)
    b.frame(msg[4128:], 0x40)
    b.frame(b"whole-2", 0xC0)
    cases = [(edge, 0, None), (edge, 0, 3), (edge, first["next"], None), (a.bytes(), 0, None), (b.bytes(), 0, None),
             (b"", 0, None), (S.decoy_block()[0], 0, None)]
    path = tmp_path / "cases.bin"
    S.write_cases(path, cases)
    subprocess.run(["make", "-s", "-C", S.DIR, "test_term_host"], check=True)
    r = subprocess.run([os.path.join(S.DIR, "test_term_host"), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "term host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict((int(k), (int(m), int(nb), int(p))) for k, m, nb, p in
                 re.findall(r"case (\d+): messages (\d+) bytes (\d+) pending (\d+)", r.stdout))
    # the spanning message: open after the first block (2752 bytes pending), delivered whole by the second
    assert lines[3][0] == 1 and lines[3][2] == 2752
    assert lines[4] == (2, 5000 + 7, 0)
