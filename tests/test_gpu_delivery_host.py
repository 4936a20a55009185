"""GPU: DeliveryTracker of the C++ host mirror (tests/delivery/test_delivery_host.cpp): batch and
single forms, ids over 40 bytes through the host sets, escaped ids equal to plain ones, growth by
rehash from 64 slots and clear_duplicate_tracking, each compared with a plain std::set / std::map
transcription of the example's callback run over the same sequence inside the program."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "delivery")


def test_delivery_tracker_against_sets_and_maps(codec):
    subprocess.run(["make", "-s", "-C", DIR, "test_delivery_host"], check=True)
    r = subprocess.run([os.path.join(DIR, "test_delivery_host")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "delivery host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
