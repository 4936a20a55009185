"""GPU: the report members of DeliveryTracker in the C++ host mirror
(tests/report/test_report_host.cpp): missing_ids, extra_ids, redelivered_ids and latency_report
after every batch and single message of one sequence, ids over 40 bytes in all three lists and
among the latency samples, the log growing by reallocation, each compared with std::set / std::map /
std::sort over the same sequence inside the program."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "report")


def test_tracker_reports_against_sets_and_sorts(codec):
    subprocess.run(["make", "-s", "-C", DIR, "test_report_host"], check=True)
    r = subprocess.run([os.path.join(DIR, "test_report_host")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "report host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
