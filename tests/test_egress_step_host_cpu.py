"""CPU: the host mirror's composed egress step exists (EgressCommitter::poll_commit_append in the
header and the library) and throws where the calls it composes throw, before anything is enqueued:
tests/egressstep/test_egress_step_host --throws needs no device."""
import os
import subprocess

import sbe_testlib as T

DIR = os.path.join(T.ROOT, "tests", "egressstep")


def test_header_and_library_have_the_entry():
    text = open(os.path.join(T.PKG, "host", "aeron_cluster_amd.hpp")).read()
    for name in ("class EgressCommitter", "poll_commit_append(", "struct EgressStepOptions", "struct EgressStepResult"):
        assert name in text, name
    r = subprocess.run(["nm", "-DC", os.path.join(T.PKG, "libaeron_cluster_amd.so")], capture_output=True, text=True, check=True)
    assert "aeron_cluster::EgressCommitter::poll_commit_append(" in r.stdout


def test_throws_where_the_base_calls_throw():
    subprocess.run(["make", "-s", "-C", DIR, "test_egress_step_host"], check=True)
    r = subprocess.run([os.path.join(DIR, "test_egress_step_host"), "--throws"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "egress step throws: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
