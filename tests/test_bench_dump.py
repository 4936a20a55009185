"""CPU: bench.py's --dump-outputs writer on a buffer set filled by the oracle — float32 / float64
files that hold the outputs exactly, a fixed sample (same indices on every call), whole-batch sums,
well under the 64 MB limit; and the command line around it (--full, --dump-outputs, --steps)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sbe_testlib as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _oracle_set(n):
    arena, L, ts = T.fixed256_orders(n)
    out, off, status = T.oracle_encode(arena, L, ts)
    d = T.oracle_decode(out, off, T.DEC_PARSE)
    seq = T.oracle_seq_batch(out, off, d)
    t = lambda a, v: torch.from_numpy(np.ascontiguousarray(a).view(v).copy())  # noqa: E731
    dec = SimpleNamespace(status=t(d["status"], np.uint8), flags=t(d["flags"], np.uint8), hdr=t(d["hdr"], np.int16),
                          ts=t(d["ts"], np.int64), view_off=t(d["view_off"], np.int32),
                          view_len=t(d["view_len"], np.int32))
    cap = out.size + 16
    buf = np.zeros(cap, np.uint8)
    buf[: out.size] = out
    b = dict(out=torch.from_numpy(buf), out_off=t(off, np.int64), status=t(status, np.uint8), dec=dec,
             seq=t(seq, np.int64))
    return b, out, off, d


@pytest.mark.parametrize("n", [1, 5000, 40000])
def test_dump_outputs_holds_the_step_outputs(tmp_path, n):
    import bench
    b, out, off, d = _oracle_set(n)
    bench.dump_outputs(str(tmp_path / "a"), b, n)
    bench.dump_outputs(str(tmp_path / "b"), b, n)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == 14
    got, size = {}, 0
    for f in names:
        assert f.endswith(".npy")
        a = np.load(tmp_path / "a" / f)
        assert a.dtype in (np.float32, np.float64), (f, a.dtype)
        assert np.array_equal(a, np.load(tmp_path / "b" / f)), f
        size += os.path.getsize(tmp_path / "a" / f)
        got[f[:-4]] = a
    assert size <= 64_000_000
    k = min(n, bench.DUMP_SAMPLE)
    idx = got["sample_index"].astype(np.int64)
    assert idx.shape == (k,) and idx[0] == 0 and idx[-1] == n - 1 and np.all(np.diff(idx) >= 0)
    assert np.array_equal(got["encoded_offset"], off[idx].astype(np.float64))
    assert np.array_equal(got["encoded_len"], (off[idx + 1] - off[idx]).astype(np.float64))
    recs = out.reshape(n, 256)[idx]
    assert np.array_equal(got["encoded_records"], recs.astype(np.float32))
    assert np.array_equal(got["encode_status"], np.zeros(k, np.float32))
    for key in ("status", "flags", "hdr", "view_off", "view_len"):
        assert np.array_equal(got["decoded_" + key], d[key][idx].astype(got["decoded_" + key].dtype)), key
    ts = got["decoded_ts_hi_lo"].astype(np.uint64)
    assert np.array_equal((ts[:, 0] << np.uint64(32)) | ts[:, 1], d["ts"][idx])
    assert not got["decoded_seq_hi_lo"].any()  # these payloads carry no _sequence_number
    sums = got["encoded_chunk_sums"]
    assert sums.size == -(-out.size // bench.DUMP_CHUNK)
    assert sums.sum() == float(out.sum(dtype=np.uint64))
    assert sums[-1] == float(out[(sums.size - 1) * bench.DUMP_CHUNK:].sum(dtype=np.uint64))
    cols = np.concatenate([[d["status"].sum(dtype=np.uint64)], [d["flags"].sum(dtype=np.uint64)],
                           d["hdr"].sum(0, dtype=np.uint64), d["view_off"].sum(0, dtype=np.uint64),
                           d["view_len"].sum(0, dtype=np.uint64)]).astype(np.float64)
    assert np.array_equal(got["decoded_column_sums"], cols)


def test_dump_outputs_shows_a_changed_byte(tmp_path):
    """A byte outside the sample still changes a file (the chunk sums cover the whole stream)."""
    import bench
    n = 40000
    b, out, off, d = _oracle_set(n)
    bench.dump_outputs(str(tmp_path / "a"), b, n)
    idx = np.load(tmp_path / "a" / "sample_index.npy").astype(np.int64)
    miss = int(np.setdiff1d(np.arange(n), idx)[0])
    b["out"][256 * miss + 100] += 1
    bench.dump_outputs(str(tmp_path / "b"), b, n)
    assert np.array_equal(np.load(tmp_path / "a" / "encoded_records.npy"), np.load(tmp_path / "b" / "encoded_records.npy"))
    assert not np.array_equal(np.load(tmp_path / "a" / "encoded_chunk_sums.npy"),
                              np.load(tmp_path / "b" / "encoded_chunk_sums.npy"))


def test_command_line(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d", "--steps", "3"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "d" and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()
