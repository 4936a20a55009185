"""CPU: the host mirror's CommitManager::serialize_commit_offset and build_commit_offset_fallback
(src/commit_manager.cpp:197-209 and :134-175) against the composition of commitfallback_lib: the
restated text, and the oracle's TopicMessage encoder in publish_topic mode for the record, with the
u16 wrap of uuid and payload and the 1040-byte [E100] bound.  The program
tests/commitfallback/test_fallback_host_cpu uses no device."""
import struct
import subprocess

import commitfallback_lib as F


def _cases():
    sk = F.skeleton_len(b"t", b"c", 0, 9)
    fixed = 63 + len(F.uuid(b"c", F.UUID0)) + sk
    c = [
        (b"gamma", b"client-7", b"m-1", 1001, 0),
        (b"default", b"", b"", 0, 0),
        (b't\x01\xc3\xa9\xf0\x9f\x98\x80/\x7f\xfe', b'z"\x01z', F.ESC_ID, 2**64 - 5, 2**64 - 1),
        (b"t", b"c", b"f" * (1040 - fixed), 9, 0),           # exactly 1040 through the id
        (b"t", b"c", b"f" * (1040 - fixed + 1), 9, 0),       # 1041: [E100]
        (b"t", b"c", b"\x01" * 65535, 9, 0),                 # the text wraps
        (b"t", b"c", b"w" * (65536 - sk), 9, 0),             # text_len mod 65536 == 0: an empty payload
        (b"t", b"c", b"w" * (65536 - sk + 1), 9, 0),
        (b"t", b"I" * 300, b"m", 9, 0),
        (b"t", b"J" * 65536, b"m", 9, 0),                    # the uuid wraps (and the text is over 65536)
        (b"t", b"J" * (65536 - 34 + 5), b"m", 9, 0),         # a uuid of 65536 + 5 bytes: 5 are stored
    ]
    # exactly 1040 and 1041 through the identifier (a plain identifier counts twice: uuid and text)
    base = 63 + len(F.uuid(b"", F.UUID0)) + F.skeleton_len(b"t", b"", 0, 9)
    mid = b"m" * (1 + (1040 - base - 1) % 2)
    L = (1040 - base - len(mid)) // 2
    c += [(b"t", b"I" * L, mid, 9, 0), (b"t", b"I" * (L - 1) + b'"', mid, 9, 0)]
    return c


def test_host_functions_match_the_composition(tmp_path):
    cases = _cases()
    fields = [F.json_fields(t, ident, mid, seq, ts, F.UUID0) for t, ident, mid, ts, seq in cases]
    assert [i for i, f in enumerate(fields) if f is None] == [4, 12]  # the two 1041-byte records
    # the last of the uuid-wrap cases stores 5 uuid bytes and a text of (len mod 65536) bytes
    assert len(F.uuid(cases[10][1], F.UUID0)) == 65536 + 5
    recs = iter(F.encode_records([f for f in fields if f is not None], F.NOW))

    def s(b):
        return struct.pack("<Q", len(b)) + b

    blob = struct.pack("<Q", len(cases))
    for (t, ident, mid, ts, seq), f in zip(cases, fields):
        blob += s(t) + s(ident) + s(mid) + struct.pack("<4Q", ts, seq, F.NOW, F.UUID0) + s(F.text(t, ident, mid, seq, ts))
        blob += struct.pack("<Q", 0) if f is None else struct.pack("<Q", 1) + s(next(recs).tobytes())
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    prog = F._make("test_fallback_host_cpu")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and f"ok ({len(cases)} cases)" in r.stdout, r.stdout + r.stderr
