"""GPU: AutoCommitter::commit_and_send_batch of the C++ host mirror (tests/commitsend/
test_commit_send_host.cpp): the CommitManager ends up as commit_record_by_record leaves it and the
offer_ingress-shaped sink receives exactly the expected frames, in record order."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_commit_and_send_host_program(codec):
    d = os.path.join(HERE, "commitsend")
    subprocess.run(["make", "-s", "-C", d, "test_commit_send_host"], check=True)
    r = subprocess.run([os.path.join(d, "test_commit_send_host")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "commit send host test: ok" in r.stdout
