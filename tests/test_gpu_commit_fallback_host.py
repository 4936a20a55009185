"""GPU: AutoCommitter::commit_and_send_batch of the C++ host mirror with json_fallback on
(tests/commitfallback/test_fallback_send_host.cpp): the sink receives every frame in record order,
device-built and host-built JSON frames equal CommitManager::build_commit_offset_fallback, `unsent`
is empty, and with the option off the results are as before."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_fallback_send_host_program(codec):
    d = os.path.join(HERE, "commitfallback")
    subprocess.run(["make", "-s", "-C", d, "test_fallback_send_host"], check=True)
    r = subprocess.run([os.path.join(d, "test_fallback_send_host")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "fallback send host test: ok" in r.stdout
