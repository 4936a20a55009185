"""GPU: the host mirror's use of sbe_order_select (tests/select/test_select_host.cpp) over the edge
batch of tests/select_lib.py and order messages in every payload format: ParsedBatch::order_select
against ParseResult::is_*() of batch.result(i), extract_order_ids(batch) against the one-record
form, DeliveryTracker::on_batch against on_message over the TopicMessage records with a fresh
tracker (the batch form selects no other record; the one-record form takes any ParseResult)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import select_lib as S

pytestmark = pytest.mark.gpu


def test_mirror_against_the_host_predicates(codec, tmp_path):
    names, data, off, dec = S.edge_case(codec.order_select_window())
    path = tmp_path / "edge.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", len(names), len(data)))
        f.write(np.ascontiguousarray(off, np.uint64).tobytes())
        f.write(np.ascontiguousarray(data, np.uint8).tobytes())
    subprocess.run(["make", "-s", "-C", S.DIR, "test_select_host"], check=True)
    r = subprocess.run([os.path.join(S.DIR, "test_select_host"), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "select host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
