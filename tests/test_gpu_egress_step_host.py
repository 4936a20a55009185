"""GPU: the host mirror's EgressCommitter::poll_commit_append (tests/egressstep/test_egress_step_host.cpp)
beside the composition that defines it: poll_term_block, MessageParser, commit_and_send_batch with
the JSON fallback, TermAppender::append of the offered frames but for the host-resolved records.
The blocks are those of test_gpu_egress_step.py's kind (fragmented messages, a message that spans
two blocks, a limit stop, an empty and an uncommitted block), polled one after another; the topics
cover CommitOffsetLite frames (topics with an id), JSON frames (table entries and plain topics
without one) and records left to the host (a number and an escaped string)."""
import os
import re
import subprocess

import pytest

import commitsend_lib as C
import sbe_testlib as T
import termscan_lib as S
from test_gpu_egress_step import put

pytestmark = pytest.mark.gpu
DIR = os.path.join(T.ROOT, "tests", "egressstep")
TOPICS = [b'"orders"', b'"alpha"', b'"user-%d"', b"12", b'"delt\\u0061"', b'"order_request_topic"', b'"orders_ack"']


def message(i):
    t = TOPICS[i % len(TOPICS)]
    hd = b'{"topic":' + (t % i if b"%d" in t else t) + b"}"
    if i % 5 == 1:
        rec = T.tm_wire([b"orders", b"SUBSCRIBE", b"s%d" % i, C.P, b"{}"], i)
    elif i % 13 == 6:
        rec = T.ack_wire(b"m%d" % i, b"orders", b"c", i)
    else:
        rec = T.tm_wire([b"orders", b"X", (b"ack_%d" if i % 17 == 3 else b"id-%d") % i, C.PSEQ if i % 4 == 0 else C.P, hd], 1_000_000 + i)
    return T.session_wrap(rec, 3, 4)


def blocks():
    a = S.Block()
    for i in range(90):
        put(a, message(i), 96 if i % 9 == 4 else None)
    tail = message(90)
    a.frame(tail[:64], 0x80)
    a.frame(tail[64:128], 0x00)
    b = S.Block()
    b.frame(tail[128:], 0x40)
    for i in range(91, 121):
        put(b, message(i), 96 if i % 9 == 2 else None)
    return a.bytes(), b.bytes()


def test_poll_commit_append_against_the_composed_calls(codec, tmp_path):
    a, b = blocks()
    first = S.walk(b, 0, 12)
    cases = [(a, 0, None), (b, 0, 12), (b, first["next"], None), (b"", 0, None), (bytes(128), 0, None), (a, 0, 40), (b, 32 * 3, 0)]
    path = tmp_path / "cases.bin"
    S.write_cases(path, cases)
    subprocess.run(["make", "-s", "-C", DIR, "test_egress_step_host"], check=True)
    r = subprocess.run([os.path.join(DIR, "test_egress_step_host"), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "egress step host: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [tuple(int(x) for x in t) for t in
             re.findall(r"case \d+: messages (\d+) frames (\d+) host (\d+) pending (\d+) next (\d+) tail (\d+)", r.stdout)]
    assert len(lines) == len(cases)
    assert lines[0][0] == 90 and lines[0][1] > 20 and lines[0][2] > 5 and lines[0][3] == min(len(message(90)), 128)
    assert 0 < lines[1][0] <= 12 and lines[2][0] > 10
    assert lines[3][:3] == (0, 0, 0) and lines[4][:3] == (0, 0, 0) and lines[6][:3] == (0, 0, 0)
    tails = [t[5] for t in lines]
    assert tails == sorted(tails) and tails[0] > 64 and tails[3] == tails[2]
    # a 4 KiB ingress block: the frames of the first block do not fit, the append trips (a padding-frame
    # header behind the last frame that fits, fewer frames appended than emitted), and so does the third
    r = subprocess.run([os.path.join(DIR, "test_egress_step_host"), str(path), "4096"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "egress step host: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    small = [tuple(int(x) for x in t) for t in
             re.findall(r"case \d+: messages \d+ frames (\d+) host \d+ pending \d+ next \d+ tail (\d+) stop (\d+) appended (\d+)", r.stdout)]
    assert len(small) == len(cases)
    assert small[0][2] == codec.TERM_APPEND_TRIPPED and small[0][1] == 4096 and 0 < small[0][3] < small[0][0]
    assert [x[2] for x in small].count(codec.TERM_APPEND_TRIPPED) >= 2
