"""GPU: the host mirror's FragmentReassembler::poll_term_block (tests/termpoll/test_termpoll_host.cpp)
beside on_term_block and term_walk + on_fragments, over the case list of test_gpu_term_host.py: the
tile-edge block whole, limited and restarted, a 5000-byte message that spans two blocks, the empty
block and the decoy block, polled one after another by one reassembler of each kind."""
import os
import re
import subprocess

import pytest

import sbe_testlib as T
import termscan_lib as S

pytestmark = pytest.mark.gpu
DIR = os.path.join(T.ROOT, "tests", "termpoll")


def test_poll_term_block_against_on_term_block(codec, tmp_path):
    t = codec.term_scan_tile()
    edge = S.tile_block(t)
    first = S.walk(edge, 0, 3)
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
             (b"", 0, None), (S.decoy_block()[0], 0, None),
             # an accumulator that meets a limit of 0, an empty block and a block it is appended to whole
             (a.bytes(), 0, None), (b.bytes(), 0, 0), (b"", 0, None), (b.bytes(), 0, 1), (b.bytes(), 32 + 1376, None)]
    path = tmp_path / "cases.bin"
    S.write_cases(path, cases)
    subprocess.run(["make", "-s", "-C", DIR, "test_termpoll_host"], check=True)
    r = subprocess.run([os.path.join(DIR, "test_termpoll_host"), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "term poll host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict((int(k), (int(m), int(nb), int(p))) for k, m, nb, p in
                 re.findall(r"case (\d+): messages (\d+) bytes (\d+) pending (\d+)", r.stdout))
    # the spanning message: open after the first block (2752 bytes pending), delivered whole by the second
    assert lines[3][0] == 1 and lines[3][2] == 2752
    assert lines[4] == (2, 5000 + 7, 0)
    assert lines[8] == (0, 0, 2752) and lines[9] == (0, 0, 2752) and lines[10] == (0, 0, 2752 + 1376)
    assert len(lines) == len(cases) + 1   # and the END frame that flushes the accumulator
