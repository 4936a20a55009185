"""GPU: the host mirror's TermAppender (tests/termappend/test_termappend_host.cpp: sbe_term_append on
the device, the written bytes copied back into a sentinel-filled host block) against the host
term_append, over the cases of tests/termappend_lib.py the device tests run too, and over an encoded
batch appended from its second record on."""
import os
import re
import subprocess

import pytest

import termappend_lib as A

pytestmark = pytest.mark.gpu


def test_append_batch_against_host_term_append(codec, tmp_path):
    cases = A.shared_cases(codec.term_append_tile())
    path = tmp_path / "cases.bin"
    A.write_cases(path, cases)
    subprocess.run(["make", "-s", "-C", A.DIR, "test_termappend_host"], check=True)
    r = subprocess.run([os.path.join(A.DIR, "test_termappend_host"), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "term append host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict((int(k), (int(a), int(n), int(s))) for k, a, n, s in
                 re.findall(r"case (\d+): appended (\d+) next (\d+) stop (\d+)", r.stdout))
    assert len(lines) == len(cases)
    for k, c in enumerate(cases):
        e = c.expect()
        assert lines[k] == (e["appended"], e["next"], e["stop"]), c.name
    assert re.search(r"batch: appended 2 next \d+ stop 0\n", r.stdout)
