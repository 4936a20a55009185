"""GPU: AckCorrelator and TopicPublisher::set_correlator of the C++ host mirror
(tests/inflight/test_inflight_host.cpp): single and batch forms, keys over 40 bytes through the
host map, a sink that refuses every third offer and growth by rehash from 64 slots, each compared
with a plain std::unordered_map run of the same sequence inside the program."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "inflight")


def test_ack_correlator_against_unordered_map(codec):
    subprocess.run(["make", "-s", "-C", DIR, "test_inflight_host"], check=True)
    r = subprocess.run([os.path.join(DIR, "test_inflight_host")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "inflight host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
