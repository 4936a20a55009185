"""CPU: the host mirror's term_walk (the second restatement of the term-buffer walk, C++) against
the Python restatement, as a stand-alone host program (tests/term/term_walk_main.cpp) over blocks
written by tests/termscan_lib.py; and the same program built with AddressSanitizer and UBSan over
the adversarial blocks, every block in a heap allocation of exactly its size."""
import os
import subprocess

import pytest

import termscan_lib as S


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("term") / "cases.bin"
    cases = S.adversarial_cases()
    S.write_cases(path, cases)
    return str(path), len(cases)


def _run(target, case_file):
    path, n = case_file
    subprocess.run(["make", "-s", "-C", S.DIR, target], check=True)
    r = subprocess.run([os.path.join(S.DIR, target), path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "term walk: %d cases ok" % n in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_term_walk_matches_the_restatement(case_file):
    _run("term_walk_check", case_file)


def test_term_walk_under_sanitizers(case_file):
    _run("term_walk_sanitize", case_file)
