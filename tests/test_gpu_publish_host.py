"""GPU: OrderPublisher of the C++ host mirror (tests/publish/test_publish_host.cpp) with an injected
id generator and clock: publish_orders_batch and single publish_order_to_topic hand the sink the
bytes the Python composition expects (oracle texts through the oracle encoder), for framed REF mode
and bare wire mode; an invalid order throws the reference's text; `misc` covers "Topic is empty",
the default id's format and a refused offer."""
import subprocess

import numpy as np
import pytest

import publish_lib as P

pytestmark = pytest.mark.gpu
TOPIC = b"order_request_topic"


def _batch():
    tab, _ = P.hand_table()
    mix = P.mixed_batch(300, 9)
    b = P.Batch(tab.fields + mix.fields, np.concatenate([tab.cid, mix.cid]), np.concatenate([tab.ts, mix.ts]),
                np.concatenate([tab.q, mix.q]), tab.order_type + mix.order_type, tab.tif + mix.tif,
                np.concatenate([tab.limit_price, mix.limit_price]), np.concatenate([tab.stop_price, mix.stop_price]),
                np.concatenate([tab.present, mix.present]))
    tm_ts = 1_760_000_000_000_000_000 + 17 * np.arange(b.n, dtype=np.uint64)
    return b, tm_ts


def _run(mode, src, dst):
    r = subprocess.run([P.binary("test_publish_host"), mode, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "publish host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return P.Parse(dst)


@pytest.mark.parametrize("session,truncate8", [(True, True), (False, False)], ids=["framed_ref", "bare_wire"])
def test_publisher_bytes(codec, tmp_path, session, truncate8):
    b, tm_ts = _batch()
    recs, _, status, mask = P.expected(b, TOPIC, tm_ts, 0, 1 if truncate8 else 0, session, term=12, sess=-3)
    want = [recs[i] for i in range(b.n) if status[i] == 0]
    assert len(want) > 30 and (status >= 16).sum() > 100
    src = str(tmp_path / "orders.bin")
    P.write_orders(src, b, TOPIC, tm_ts, session, truncate8, 12, -3)
    out = _run("batch", src, str(tmp_path / "batch.bin"))
    got = [out.string() for _ in range(out.u32())]
    assert got == want
    assert np.array_equal(np.frombuffer(out.take(b.n), np.uint8), status)
    assert np.array_equal(np.frombuffer(out.take(2 * b.n), np.uint16), mask)
    assert [out.string() for _ in range(b.n)] == [f[P.F_MSGID] for f in b.fields] and out.done()
    # one publish_order_to_topic per order (the first 60: one device call each)
    k = 60
    one = P.Batch(b.fields[:k], b.cid[:k], b.ts[:k], b.q[:k], b.order_type[:k], b.tif[:k], b.limit_price[:k],
                  b.stop_price[:k], b.present[:k])
    P.write_orders(src, one, TOPIC, tm_ts[:k], session, truncate8, 12, -3)
    out = _run("single", src, str(tmp_path / "single.bin"))
    got = [out.string() for _ in range(out.u32())]
    assert got == [recs[i] for i in range(k) if status[i] == 0]
    for i in range(k):
        kind, text = out.take(1)[0], out.string()
        if status[i] == 0:
            assert (kind, text) == (0, b.fields[i][P.F_MSGID])
        else:
            first = int(status[i]) - 16
            tail = b.order_type[i] if first == 5 else b.tif[i] if first == 10 else b""
            want_text = b"Invalid message: Order validation failed: " + P.MESSAGES[first].encode() + tail
            # the program reports what(), a C string: a NUL inside order_type / time_in_force ends it
            assert kind == 1 and text == want_text.split(b"\0")[0], (i, text)
    assert out.done()


def test_publisher_misc(codec):
    r = subprocess.run([P.binary("test_publish_host"), "misc"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "publish host misc: ok" in r.stdout, r.stdout + r.stderr
