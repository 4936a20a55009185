"""CPU: the piece location of sbe_term_poll's gather (csrc/term_poll_locate.hpp: the fragment walk
the kernel runs for entries of several fragments, under the serial form of its search and entry
loop, whose device forms the GPU tests cover) as a stand-alone host program (tests/termpoll/term_poll_locate_main.cpp):
over the adversarial blocks of tests/termscan_lib.py and the long-message, scan-block-edge and carry
blocks of the GPU test, every output gathered in pieces of 64, 1024 and the shipped size equals a
serial reassembly; and the same program built with AddressSanitizer and UBSan, block, carry and
output each in a heap allocation of exactly its size."""
import os
import subprocess

import pytest

import sbe_testlib as T
import termpoll_lib as P
import termscan_lib as S

DIR = os.path.join(T.ROOT, "tests", "termpoll")
CARRIES, PIECES = 5, 3   # what the program runs every case with


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("termpoll") / "cases.bin"
    cases = P.host_cases()
    S.write_cases(path, cases)
    return str(path), len(cases)


def _run(target, case_file):
    path, n = case_file
    subprocess.run(["make", "-s", "-C", DIR, target], check=True)
    r = subprocess.run([os.path.join(DIR, target), path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "term poll locate: %d gathers ok" % (n * CARRIES * PIECES) in r.stdout, \
        r.stdout[-2000:] + r.stderr[-4000:]


def test_piece_location_gathers_every_message(case_file):
    _run("term_poll_locate_check", case_file)


def test_piece_location_under_sanitizers(case_file):
    _run("term_poll_locate_sanitize", case_file)


def test_reference_composition_of_the_shared_blocks():
    """The blocks reach the branches they are built for (a change of a builder cannot quietly empty one)."""
    t = 32768
    e = P.expect(P.long_block(t))
    assert [len(x) for x in e["msgs"]] == [6, 0, 200000, 5, 33] and e["carry"] == b""
    src = e["walk"]["frag_src"]
    assert src[2] < t and src[-3] > 6 * t                       # the message crosses tile edges
    assert [len(x) for x in P.expect(P.long_block(t, True))["msgs"]] == [6, 0, 25, 200000, 5, 33]
    limit, prefix = P.open_limit()
    e = P.expect(P.long_block(t), 0, limit)
    assert len(e["msgs"]) == 2 and len(e["carry"]) == prefix >= 100000 and e["counts"][3] == S.LIMIT
    e = P.expect(P.edge_group_block(1000))
    fl = e["walk"]["flags"]
    assert fl[1000] == 0x80 and fl.index(0x40) > 1024 and 0xC0 in fl[1001:1024] and 0xC0 in fl[1025:fl.index(0x40)]
    assert len(e["msgs"]) == 1000 + 30 + 1 + 1
