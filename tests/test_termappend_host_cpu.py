"""CPU: the host mirror's term_append (the second restatement of the publish-side framing, C++)
against the Python restatement, as a stand-alone host program (tests/termappend/term_append_main.cpp)
over the case file tests/termappend_lib.py writes; and the same program built with AddressSanitizer
and UBSan over the same cases (malformed offsets and trips among them), the block and the input
each in a heap allocation of exactly its size."""
import os
import subprocess

import pytest

import termappend_lib as A


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("termappend") / "cases.bin"
    cases = A.shared_cases()
    A.write_cases(path, cases)
    return str(path), len(cases)


def _run(target, case_file):
    path, n = case_file
    subprocess.run(["make", "-s", "-C", A.DIR, target], check=True)
    r = subprocess.run([os.path.join(A.DIR, target), path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "term append: %d cases ok" % n in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_term_append_matches_the_restatement(case_file):
    _run("term_append_check", case_file)


def test_term_append_under_sanitizers(case_file):
    _run("term_append_sanitize", case_file)
