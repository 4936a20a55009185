"""Per-row measurement of the SURVEY §8 rows beyond the headline bench: one JSON line per workload
with records/s (whole calls, device-resident), each dominant kernel's HIP-event duration, its
algorithmic bytes per launch (computed from the actual record sizes) and its fraction of the
8 TB/s HBM peak.  Rows:
  config3_mixed_decode   1 M mixed TopicMessage / Ack records, parse_message
  config4_var_roundtrip  16 M variable-length TopicMessages, encode + parse decode (config 4)
  session_fixed256       1 M session-framed Order TopicMessages (32-B SessionMessageHeader + 248 B)
  lite301 / lite201      1 M CommitOffsetLite / OrderRequestLite records, encode + Lite decode
  order_json             1 M Orders → Order::to_json payload + publish_order headers JSON (two calls)
  publish_orders         1 M Orders → session-framed REF-mode wire records in one fused call
                         (sbe_publish_orders_batch), and in the same run the composed path it replaces:
                         the two order_json calls plus sbe_encode_session_batch on prepared offsets
  reassemble             1 M Aeron fragments (90 % whole messages, the rest BEGIN..END groups),
                         BEGIN/END reassembly (all its launches, torch events around the call)
  materialize            1 M fixed-256 records' parse_message views copied into one arena
                         (sbe_materialize_views, all its launches, torch events around the call)
  commit_emit            1 M decoded and classified fixed-256 Orders, all committed → session-framed
                         CommitOffsetLite frames in one fused call (sbe_emit_commit_offsets), and in the
                         same run sbe_encode_lite_batch on a pre-gathered arena of the same ids
  commit_fallback        the commit_emit batch with a table whose entries all have id 0 → session-framed
                         JSON COMMIT_OFFSET TopicMessages (sbe_emit_commit_offsets_ex with a fallback)
  json_extract           1 M decoded fixed-256 Orders, the nine order-id member paths read out of every
                         payload (sbe_json_extract_batch), flat and nested payloads, and in the same run
                         sbe_classify_commits on the same buffers (same staging, no record parsed)
  order_select           1 M decoded fixed-256 Orders, the ParseResult predicates, the subscriber's order test
                         and the topic class per record (sbe_order_select): CREATE_ORDER types (no payload
                         searched) and an empty type with nested payloads (every payload searched), and the
                         host loop over ParseResults it replaces, timed on the CPU in the same row
  term_scan              a raw 16 MiB term-buffer block (config-3 records, session-framed, long messages in
                         frames of at most 1376 bytes) framed on the device (sbe_term_scan): the scan alone,
                         tables only, scan + reassembly, a device copy of the payload as the ceiling, and the
                         host mirror's one-thread term_walk with its payload memcpy
  term_poll              the same block polled into whole messages by one call (sbe_term_poll), and the chain
                         it replaces (sbe_term_scan with payload copy + sbe_reassemble_fragments), twice
  term_append            the records of that block (built first, encoded in device memory) appended to a 16 MiB
                         term-buffer block with Aeron's framing at MTU 1408 on the device (sbe_term_append),
                         a device copy of the same payload bytes as the ceiling, and the host mirror's
                         one-thread term_append
  egress_step            a raw 16 MiB block of session-framed fixed-256 Orders through the whole egress step
                         (poll, decode, classify, emit, append of the commit frames): egress_commit_step as
                         one enqueue with the counts on the device, and the uncounted calls with their two
                         host reads on the same inputs; then sbe_decode_batch_counted beside
                         sbe_decode_batch_sized on 1 M records at count == capacity and capacity / 16
  ack_correlate          1 M "pub_<nanos>" uuids remembered in a 2 M-slot in-flight table, then 1 M full
                         acks (about 10 % unknown ids, 1 % repeated ids) decoded on-egress and matched;
                         remember, match and the decode of the same ack batch timed in the same run, and
                         a one-thread std::unordered_map doing the same sequence on the host
  delivery_track         1 M decoded fixed-256 Orders with nested payloads, about 10 % of them redeliveries,
                         against 2 M-slot tables and 1 M sent client order ids: sbe_delivery_keys, note
                         (message ids), note (client ids) and lookup (sent) timed as one region, the
                         nine-path extract before it timed beside it, and a one-thread std::set /
                         std::map run of the example's callback on the host
  delivery_report        the reports read from those sets: 2 M-slot sent and received tables with 1 M sent
                         ids, about 1 % never received and 1 % of the received never sent, and a log of
                         1 M latencies: sbe_inflight_list_keys both ways (limit 10) and
                         sbe_latency_report (seven percentiles, order) timed as one region, and a
                         one-thread std::set / std::sort run of the example's reports on the host
Rows whose buffers fit the 256 MB MALL a few times over rotate over --rotate (3) copies of their
inputs and outputs (step k uses copy k mod R), as bench.py does, so no step finds its inputs in the
cache a previous step left them in; config 4's 16.8 M-record batch (~6.5 GB) needs no rotation.
Usage: python scripts/bench_rows.py [--steps K] [--rows a,b,...] [--rotate R]  (GPU only)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "aeron-cluster-client-cpp_amd"), os.path.join(ROOT, "tests")]
import sbe_testlib as T  # noqa: E402
import sbecodec  # noqa: E402

PEAK = 8000.0
DESC = 1 + 1 + 8 + 8 + 40  # decode descriptor bytes written per record


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view({torch.uint8: np.uint8, torch.int32: np.int32,
                                                           torch.int64: np.int64}[dt])).to("cuda")


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    sbecodec.profile_enable(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    pack = sbecodec.profile_read(sbecodec.PROF_PACK)
    deck = sbecodec.profile_read(sbecodec.PROF_DECODE)
    sbecodec.profile_enable(0)
    return el / steps, (float(np.mean(pack)) if pack else None), (float(np.mean(deck)) if deck else None)


ROT = 3  # --rotate


class Rot:
    """R copies of a row's device buffers; next() is the copy for the next step."""

    def __init__(self, make):
        self.sets = [make(k) for k in range(max(ROT, 1))]
        self.k = 0

    def next(self):
        x = self.sets[self.k % len(self.sets)]
        self.k += 1
        return x


CPU_THREADS = 16
CPU_SECONDS = 3.0
NO_CPU = False  # --no-cpu: skip the CPU baselines (profiling runs)


def cpu_rate(fn, n_sample, budget=CPU_SECONDS):
    """records/s of fn() (the oracle restatement of the row on an n_sample-record slice of the same
    workload) repeated for about `budget` seconds on the host cores."""
    if NO_CPU:
        return None
    fn()
    done, t0 = 0, time.perf_counter()
    while True:
        fn()
        done += n_sample
        el = time.perf_counter() - t0
        if el >= budget:
            return done / el


_cpu = None


def line(row, n, step_s, kernels):
    global _cpu
    out = {"row": row, "records": n, "records_per_s": n / step_s, "ms_per_step": step_s * 1e3,
           "input_sets": 1 if row == "config4_var_roundtrip" else max(ROT, 1), "kernels": {}}
    if _cpu is not None:
        out["cpu_baseline"] = _cpu
        _cpu = None
    for name, (ms, nbytes) in kernels.items():
        if ms is None:
            continue
        gbs = nbytes / (ms * 1e-3) / 1e9
        out["kernels"][name] = {"ms": ms, "alg_bytes": nbytes, "GBps": gbs, "frac": gbs / PEAK}
    print(json.dumps(out), flush=True)


def set_cpu(value, sample, cores=CPU_THREADS):
    global _cpu
    if value is None:
        return
    _cpu = {"value": value, "unit": "records/s", "cores": cores, "kind": "port", "sample": sample}


def row_mixed(steps, warmup):
    n = 1_000_000
    data, off = T.mixed_records(n)
    d0, o0 = dev(data, torch.uint8), dev(off.astype(np.uint64), torch.int64)
    R = Rot(lambda k: (d0.clone(), o0.clone(), sbecodec.alloc_decoded(n, "cuda")))
    nb = int(off[-1])

    def step():
        d, o, out = R.next()
        sbecodec.decode_batch(d, o, sbecodec.DEC_PARSE_MESSAGE, out=out, in_bytes=nb)

    s, _, dk = timed(step, steps, warmup)
    k = 200_000
    dk_, ok_ = data[: int(off[k])], off[: k + 1]
    set_cpu(cpu_rate(lambda: T.oracle_decode(dk_, ok_, T.DEC_PARSE, nthreads=CPU_THREADS), k),
            f"{k} records of the same mix, oracle parse_message, OpenMP {CPU_THREADS} threads")
    line("config3_mixed_decode", n, s, {"sbe_decode_kernel<parse_message>": (dk, int(off[-1]) + 8 * n + DESC * n)})


def row_var(steps, warmup):
    n = 16_777_216
    a, l, t = T.var_orders_t(n, "cuda")  # == T.var_orders(n), generated on the device
    cap = sbecodec.output_bound(n, a.numel())
    ob = torch.empty(cap, dtype=torch.uint8, device="cuda")
    oo = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    ws = sbecodec.alloc_workspace(n, "cuda")
    dec = sbecodec.alloc_decoded(n, "cuda")
    outb = int(a.numel()) + 34 * n  # the stream's bytes (every record encodable)

    def step():
        sbecodec.encode_topic_batch(a, l, t, out=ob, out_off=oo, status=st, workspace=ws)
        sbecodec.decode_batch(ob, oo, sbecodec.DEC_PARSE_MESSAGE, out=dec, in_bytes=outb)

    s, pk, dk = timed(step, steps, warmup)
    k = 200_000
    ak, Lk, tk = T.var_orders(k)

    def cpu_rt():
        o, oo_, _ = T.oracle_encode(ak, Lk, tk, nthreads=CPU_THREADS)
        T.oracle_decode(o, oo_, T.DEC_PARSE, nthreads=CPU_THREADS)

    set_cpu(cpu_rate(cpu_rt, k), f"{k} variable-length records, oracle encode + parse_message, OpenMP {CPU_THREADS} threads")
    line("config4_var_roundtrip", n, s, {"sbe_enc_pack<packed,wire>": (pk, a.numel() + 28 * n + outb + 9 * n),
                                         "sbe_decode_kernel<parse_message>": (dk, outb + 8 * n + DESC * n)})


def row_session(steps, warmup):
    n = 1_000_000
    arena, L, ts = T.fixed256_orders(n)
    a0, l0, t0 = dev(arena, torch.uint8), dev(L.view(np.int32), torch.int32), dev(ts.view(np.int64), torch.int64)
    ws = sbecodec.alloc_workspace(n, "cuda")
    R = Rot(lambda k: (a0.clone(), l0.clone(), t0.clone(),
                       torch.empty(sbecodec.output_bound(n, arena.size), dtype=torch.uint8, device="cuda"),
                       torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                       torch.empty(n, dtype=torch.uint8, device="cuda"), sbecodec.alloc_decoded(n, "cuda")))

    def step():
        a, l, t, ob, oo, st, dec = R.next()
        sbecodec.encode_session_batch(a, l, t, 7, 8, out=ob, out_off=oo, status=st, workspace=ws)
        sbecodec.decode_batch(ob, oo, sbecodec.DEC_PARSE_MESSAGE, out=dec, in_bytes=n * (32 + 248))

    s, pk, dk = timed(step, steps, warmup)
    rec = 32 + 248
    k = 200_000
    ak, Lk, tk = arena[: 222 * k], L[:k], ts[:k]

    def cpu_rt():
        o, oo_, _ = T.oracle_encode_session(ak, Lk, tk, 7, 8, flags=T.ENC_REF_TRUNCATE8, nthreads=CPU_THREADS)
        T.oracle_decode(o, oo_, T.DEC_PARSE, nthreads=CPU_THREADS)

    set_cpu(cpu_rate(cpu_rt, k), f"{k} records, oracle session encode + parse_message, OpenMP {CPU_THREADS} threads")
    line("session_fixed256", n, s, {"sbe_enc_pack<session,packed,ref>": (pk, n * (222 + 28 + rec + 9)),
                                    "sbe_decode_kernel<parse_message>": (dk, n * (rec + 8 + DESC))})


def row_lite(t_id, steps, warmup):
    n = 1_000_000
    nf = T.LITE_NF[t_id]
    arena, L, tid, seq = T.lite_records(n, t_id)
    a0, l0 = dev(arena, torch.uint8), dev(L.view(np.int32), torch.int32)
    ti0, sq0 = dev(tid.view(np.int32), torch.int32), dev(seq.view(np.int64), torch.int64)
    cap = arena.size + (20 + 2 * nf) * n + 16
    ws = sbecodec.alloc_workspace(n, "cuda")
    outb = arena.size + (20 + 2 * nf) * n
    R = Rot(lambda k: (a0.clone(), l0.clone(), ti0.clone(), sq0.clone(),
                       torch.empty(cap, dtype=torch.uint8, device="cuda"),
                       torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                       torch.empty(n, dtype=torch.uint8, device="cuda"), sbecodec.alloc_decoded(n, "cuda")))

    def step():
        a, l, ti, sq, ob, oo, st, dec = R.next()
        sbecodec.encode_lite_batch(t_id, a, l, ti, sq, out=ob, out_off=oo, status=st, workspace=ws)
        sbecodec.decode_batch(ob, oo, sbecodec.DEC_LITE, out=dec, in_bytes=outb)

    s, pk, dk = timed(step, steps, warmup)
    k = 200_000
    ak, Lk, tk, sk = T.lite_records(k, t_id)

    def cpu_rt():
        o, oo_, _ = T.oracle_encode_lite(t_id, ak, Lk, tk, sk, nthreads=CPU_THREADS)
        T.oracle_decode(o, oo_, T.DEC_LITE, nthreads=CPU_THREADS)

    set_cpu(cpu_rate(cpu_rt, k), f"{k} records, oracle Lite encode + decode, OpenMP {CPU_THREADS} threads")
    line(f"lite{t_id}", n, s, {f"sbe_enc_pack<lite{nf},packed>": (pk, arena.size + (4 * nf + 12) * n + outb + 9 * n),
                               "sbe_decode_kernel<lite>": (dk, outb + 8 * n + DESC * n)})


def row_reassemble(steps, warmup):
    n = 1_000_000
    # 90 % whole messages, 10 % BEGIN..END groups of 2-5 fragments, no strays
    data, off, flags = T.fragment_stream(n, 11, p_single=0.9, maxlen=512, p_group=0.1)
    d0, o0, f0 = dev(data, torch.uint8), dev(off.view(np.int64), torch.int64), dev(flags, torch.uint8)
    ws = torch.empty(int(sbecodec.lib().sbe_reassemble_workspace_size(n)), dtype=torch.uint8, device="cuda")
    R = Rot(lambda k: (d0.clone(), o0.clone(), f0.clone(), torch.empty(max(data.size, 16), dtype=torch.uint8, device="cuda"),
                       torch.empty(n + 1, dtype=torch.int64, device="cuda")))

    def fn():
        d, o, f, out, mo = R.next()
        sbecodec.reassemble(d, o, f, out=out, msg_off=mo, workspace=ws)
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    nbytes = 2 * data.size + (8 + 1 + 8) * n  # payload read + written, frag_off + flags read, msg_off written
    k = 200_000
    dk_, ok_, fk_ = data[: int(off[k])], np.ascontiguousarray(off[: k + 1]), np.ascontiguousarray(flags[:k])
    ob_, ab_ = np.zeros(int(off[k]) + 1, np.uint8), np.zeros(int(off[k]) + 1, np.uint8)
    mo_, cn_ = np.zeros(k + 1, np.uint64), np.zeros(2, np.uint64)
    P = T._p
    set_cpu(cpu_rate(lambda: T.oracle().orc_reassemble(P(dk_), P(ok_), P(fk_), k, P(ob_), P(mo_), P(cn_), P(ab_)), k),
            f"{k} fragments of the same stream, oracle LocalFragmentReassembler restatement, 1 thread (sequential by definition)",
            cores=1)
    line("reassemble", n, ms * 1e-3, {"sbe_reassemble_fragments (all launches)": (ms, nbytes)})


def row_order_json(steps, warmup):
    n = 1_000_000
    fields, cid, ts, q = T.realistic_orders(n)
    arena, str_len = T.pack_order_fields(fields)
    args0 = (dev(arena, torch.uint8), dev(str_len.astype(np.int32), torch.int32), dev(cid, torch.int64),
             dev(ts, torch.int64), torch.from_numpy(q).cuda())

    def make(k):
        args = tuple(x.clone() for x in args0)
        outs = {w: sbecodec.order_to_json_batch(*args, what=w)
                for w in (sbecodec.JSON_ORDER_PAYLOAD, sbecodec.JSON_PUBLISH_HEADERS)}
        return args, outs

    R = Rot(make)
    outs = R.sets[0][1]

    def fn():
        args, os_ = R.next()
        for w in os_:
            sbecodec.order_to_json_batch(*args, what=w, out=os_[w].out, out_off=os_[w].out_off, status=os_[w].status)
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    text = sum(int(outs[w].out_off[-1]) for w in outs)
    # strings read (payload reads uuid / base twice), lengths + numbers read, text + offsets written
    sl = str_len.astype(np.int64)
    nbytes = int(2 * sl[:, 0].sum() + sl[:, 1:5].sum() + sl[:, 2].sum() + sl[:, 5:8].sum()) + n * (32 + 24) + \
        text + 2 * 8 * n
    k = 100_000
    ak, lk = T.pack_order_fields(fields[:k])
    set_cpu(cpu_rate(lambda: [T.oracle_order_json(ak, lk, cid[:k], ts[:k], q[:k], w, nthreads=CPU_THREADS)
                              for w in (0, 1)], k),
            f"{k} Orders of the same batch, oracle payload + headers JSON (glibc snprintf), OpenMP {CPU_THREADS} threads")
    line("order_json", n, ms * 1e-3, {"sbe_order_to_json_batch x2 (payload + headers)": (ms, nbytes)})


def row_materialize(steps, warmup):
    """MATERIALIZE (sbe_materialize_views) after a parse_message decode of 1 M fixed-256 records:
    every record's views copied into one arena (Σlen read and written, plus the
    descriptors' offsets and lengths and rec_off read and 40 B of arena offsets written a record)."""
    n = 1_000_000
    arena, L, ts = T.fixed256_orders(n)
    data, off, _ = T.oracle_encode(arena, L, ts)
    d0, o0 = dev(data, torch.uint8), dev(off.astype(np.uint64), torch.int64)
    ws = torch.empty(int(sbecodec.lib().sbe_materialize_workspace_size(n)) + 16, dtype=torch.uint8, device="cuda")

    def make(k):
        d, o = d0.clone(), o0.clone()
        dec = sbecodec.decode_batch(d, o, sbecodec.DEC_PARSE_MESSAGE, out=sbecodec.alloc_decoded(n, "cuda"),
                                    in_bytes=data.size)
        return d, o, dec, torch.empty(data.size, dtype=torch.uint8, device="cuda"), \
            torch.empty(5 * n + 1, dtype=torch.int64, device="cuda")
    R = Rot(make)
    torch.cuda.synchronize()
    vbytes = int(R.sets[0][2].view_len[:n].to(torch.int64).sum().item())

    def fn():
        d, o, dec, ar, ao = R.next()
        sbecodec.materialize_views(d, o, dec, arena=ar, arena_capacity=ar.numel(), arena_off=ao, workspace=ws)
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    nbytes = 2 * vbytes + (40 + 8 + 40) * n
    k = 200_000
    dk = T.oracle_decode(data[: int(off[k])], off[: k + 1], T.DEC_PARSE, nthreads=CPU_THREADS)
    set_cpu(cpu_rate(lambda: T.oracle_materialize(data[: int(off[k])], off[: k + 1], dk), k),
            f"{k} records of the same batch, the oracle's view copy (numpy gather), 1 thread", cores=1)
    line("materialize", n, ms * 1e-3, {"sbe_materialize_views (all launches)": (ms, nbytes)})


def _event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def row_publish_orders(steps, warmup):
    """publish_order for 1 M realistic Orders, session-framed, REF mode: the fused call
    (sbe_publish_orders_batch, validation included) and, in the same run, the composed path (two
    sbe_order_to_json_batch calls, then sbe_encode_session_batch over a prepared 5-field offset table
    into an arena that already holds both texts), device time only (torch events).  Bytes of the
    fused call: Order strings (uuid / base read twice, message_id and id twice, status), checks
    strings, 32 + 24 + 8 + 24 B of lengths and numbers read, records + offsets + status + mask
    written; the composed path moves the two texts three times more (written, read, written)."""
    n = 1_000_000
    fields, cid, ts, q = T.realistic_orders(n)
    arena, str_len = T.pack_order_fields(fields)
    topic = b"orders"
    tm_ts = (1_760_000_000_000_000_000 + np.arange(n)).astype(np.int64)
    args0 = (dev(arena, torch.uint8), dev(str_len.astype(np.int32), torch.int32), dev(cid, torch.int64),
             dev(ts, torch.int64), torch.from_numpy(q).cuda())
    topic_d = dev(np.frombuffer(topic, np.uint8), torch.uint8)
    chk0 = (dev(np.frombuffer(b"LIMITGTC" * n, np.uint8), torch.uint8),
            dev(np.tile(np.array([5, 3], np.int32), n), torch.int32), torch.ones(n, dtype=torch.float64, device="cuda"),
            torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"))
    tm0 = dev(tm_ts, torch.int64)

    def make(k):
        args = tuple(x.clone() for x in args0)
        chk = tuple(x.clone() for x in chk0)
        tm = tm0.clone()
        fused = sbecodec.publish_orders_batch(*args, topic_d, checks=chk, tm_timestamp=tm, leadership_term_id=7,
                                              cluster_session_id=9)
        P = sbecodec.order_to_json_batch(*args, what=sbecodec.JSON_ORDER_PAYLOAD)
        H = sbecodec.order_to_json_batch(*args, what=sbecodec.JSON_PUBLISH_HEADERS)
        # prepared once: topic, messageType, message ids and both texts in one arena, [n][5] offsets
        pt, ht = int(P.out_off[-1]), int(H.out_off[-1])
        ids = np.frombuffer(b"".join(f[6] for f in fields), np.uint8)
        idl = str_len[:, 6].astype(np.int64)
        big = torch.cat([topic_d, dev(np.frombuffer(b"CREATE_ORDER", np.uint8), torch.uint8), dev(ids, torch.uint8),
                         P.out[:pt], H.out[:ht]])
        b_ids = len(topic) + 12
        b_pay = b_ids + ids.size
        po, ho = P.out_off.cpu().numpy(), H.out_off.cpu().numpy()
        off, ln = np.zeros((n, 5), np.int64), np.zeros((n, 5), np.int64)
        ln[:, 0], off[:, 1], ln[:, 1] = len(topic), len(topic), 12
        off[:, 2], ln[:, 2] = b_ids + np.cumsum(idl) - idl, idl
        off[:, 3], ln[:, 3] = b_pay + po[:-1], np.diff(po)
        off[:, 4], ln[:, 4] = b_pay + pt + ho[:-1], np.diff(ho)
        enc_in = (big, dev(ln.astype(np.int32), torch.int32), tm)
        enc_off = dev(off.astype(np.uint32).view(np.int32), torch.int32)
        # topic and messageType are shared by all records, so the arena size does not bound the stream
        enc = sbecodec.encode_session_batch(*enc_in, 7, 9, str_off=enc_off,
                                            out=torch.empty(int(fused.out_off[-1]) + 64, dtype=torch.uint8, device="cuda"))
        ws = torch.empty(sbecodec.publish_orders_workspace_size(n), dtype=torch.uint8, device="cuda")
        return args, chk, tm, (fused, ws), P, H, enc_in, enc_off, enc

    R = Rot(make)
    torch.cuda.synchronize()
    _, _, _, (fused0, _), P0, H0, _, _, enc0 = R.sets[0]
    total = int(fused0.out_off[-1])
    # the two paths produce the same stream
    assert total == int(enc0.out_off[-1]) and torch.equal(fused0.out[:total], enc0.out[:total])
    assert int(fused0.status[:n].max()) == 0 and int(enc0.status[:n].max()) == 0

    def fused_fn():
        args, chk, tm, (f, ws), *_ = R.next()
        sbecodec.publish_orders_batch(*args, topic_d, checks=chk, tm_timestamp=tm, leadership_term_id=7,
                                      cluster_session_id=9, out=f.out, out_off=f.out_off, status=f.status,
                                      error_mask=f.error_mask, workspace=ws)

    def composed_fn():
        args, _, _, _, P, H, enc_in, enc_off, enc = R.next()
        sbecodec.order_to_json_batch(*args, what=sbecodec.JSON_ORDER_PAYLOAD, out=P.out, out_off=P.out_off,
                                     status=P.status)
        sbecodec.order_to_json_batch(*args, what=sbecodec.JSON_PUBLISH_HEADERS, out=H.out, out_off=H.out_off,
                                     status=H.status)
        sbecodec.encode_session_batch(*enc_in, 7, 9, str_off=enc_off, out=enc.out, out_off=enc.out_off,
                                      status=enc.status, workspace=enc.workspace)

    ms_f = _event_ms(fused_fn, steps, warmup)
    ms_c = _event_ms(composed_fn, steps, warmup)
    ms_f2 = _event_ms(fused_fn, steps, warmup)  # again after the composed path: drift between the two shows here
    text = int(P0.out_off[-1]) + int(H0.out_off[-1])
    sl = str_len.astype(np.int64)
    strings = int(2 * sl[:, 0].sum() + sl[:, 1:5].sum() + sl[:, 2].sum() + 2 * sl[:, 5:7].sum() + 2 * sl[:, 7].sum())
    nb_f = strings + 8 * n + n * (32 + 24 + 8 + 8 + 17) + total + n * (8 + 1 + 2)
    nb_c = nb_f + 3 * text
    if max(ms_f, ms_f2) > ms_c:  # the row's condition: the fused call is not slower than the path it replaces
        print(f"WARNING publish_orders: fused {ms_f:.4f} / {ms_f2:.4f} ms is slower than composed {ms_c:.4f} ms",
              file=sys.stderr, flush=True)
    print(json.dumps({"row": "publish_orders", "fused_not_slower_than_composed": bool(max(ms_f, ms_f2) <= ms_c),
                      "composed_over_fused": ms_c / ms_f}), flush=True)
    line("publish_orders", n, ms_f * 1e-3,
         {"sbe_publish_orders_batch (fused: all launches)": (ms_f, nb_f),
          "sbe_publish_orders_batch (fused, measured again after the composed path)": (ms_f2, nb_f),
          "composed: sbe_order_to_json_batch x2 + sbe_encode_session_batch (prepared offsets)": (ms_c, nb_c)})


def row_autocommit(steps, warmup):
    """sbe_classify_commits after a parse_message decode, three 1 M-record batches: fixed-256 Orders
    (no source holds "topic" or a backslash: no record is parsed), the config-3 mix, and fixed-256
    Orders whose headers all carry "topic" (every lane runs the JSON reader).  Bytes: views 1..4
    read, 42 B of descriptors (rec_off 8, status 1, flags 1, four view offsets and lengths 32) and
    15 B of outputs a record.  The fixed-256 batch also times the decode of the same
    buffers in the same run (decode reads the same record bytes)."""
    n = 1_000_000
    arena, L, ts = T.fixed256_orders(n)
    fixed = T.oracle_encode(arena, L, ts)[:2]
    worst_arena = arena.reshape(n, 222).copy()
    worst_arena[:, 190:] = np.frombuffer(b'{"topic":"orders","a":"CREATE"} ', np.uint8)
    worst = T.oracle_encode(worst_arena.reshape(-1), L, ts)[:2]
    topics = [b"orders", b"order_request_topic", b"order_notification_topic"]
    for name, (data, off) in (("fixed256", fixed), ("config3_mixed", T.mixed_records(n)), ("all_parse", worst)):
        d0, o0 = dev(data, torch.uint8), dev(np.asarray(off, np.uint64), torch.int64)
        table = sbecodec.commit_topic_table(topics, "cuda")

        def make(k):
            d, o = d0.clone(), o0.clone()
            dec = sbecodec.decode_batch(d, o, sbecodec.DEC_PARSE_MESSAGE, out=sbecodec.alloc_decoded(n, "cuda"),
                                        in_bytes=data.size)
            return d, o, dec, sbecodec.classify_commits(d, o, dec, table)
        R = Rot(make)
        torch.cuda.synchronize()
        dec0, plan0 = R.sets[0][2], R.sets[0][3]
        tm = dec0.status[:n] == 0
        vbytes = int((dec0.view_len[:n, 1:].to(torch.int64).sum(dim=1) * tm).sum().item())
        cm = np.bincount(plan0.numpy()["cm"], minlength=8).tolist()

        def fn():
            d, o, dec, plan = R.next()
            sbecodec.classify_commits(d, o, dec, table, out=plan)
        ms = _event_ms(fn, steps, warmup)
        kernels = {"sbe_classify_commits (init + classify)": (ms, vbytes + (42 + 15) * n)}
        if name == "fixed256":
            def dfn():
                d, o, dec, _ = R.next()
                sbecodec.decode_batch(d, o, sbecodec.DEC_PARSE_MESSAGE, out=dec, in_bytes=data.size)
            dms = _event_ms(dfn, steps, warmup)
            kernels["sbe_decode_batch (same buffers, same run)"] = (dms, int(off[-1]) + 8 * n + DESC * n)
        line(f"autocommit_{name}", n, ms * 1e-3, kernels)
        print(json.dumps({"row": f"autocommit_{name}", "cm_counts": cm}), flush=True)
        del R
        torch.cuda.empty_cache()


def row_json_extract(steps, warmup):
    """sbe_json_extract_batch after a parse_message decode of 1 M fixed-256 Orders, the nine
    order-id paths of examples/pubsub_reconnect_test.cpp:576-620 over the payloads: the suite's flat
    payload (every record is parsed whole, no path is found) and a nested payload of the same 143
    bytes in Order::to_json's shape (five of the nine paths are found).  Every selected record is
    parsed, so beside each the same run times sbe_classify_commits on the same buffers: the same
    staging, but no record of these batches reaches its reader.  Bytes: the payload read, 18 B of
    descriptors (rec_off 8, status 1, flags 1, one view offset and length 8) and 2 + 9 P B of
    outputs a record."""
    n = 1_000_000
    arena, L, ts = T.fixed256_orders(n)
    nested = (b'{"uuid":"cid_0123456789abcdefg","message":{"message":{"order_details":'
              b'{"client_order_id":"cid_0123456789abcdefg"}}}}')
    assert len(nested) <= 143, len(nested)
    hit_arena = arena.reshape(n, 222).copy()
    hit_arena[:, 47:190] = np.frombuffer(nested.ljust(143), np.uint8)
    paths = sbecodec.json_path_table(sbecodec.ORDER_ID_PATHS)
    topics = [b"orders", b"order_request_topic", b"order_notification_topic"]
    for name, ar in (("fixed256", arena), ("fixed256_nested", hit_arena.reshape(-1))):
        data, off = T.oracle_encode(ar, L, ts)[:2]
        d0, o0 = dev(data, torch.uint8), dev(np.asarray(off, np.uint64), torch.int64)
        table = sbecodec.commit_topic_table(topics, "cuda")

        def make(k):
            d, o = d0.clone(), o0.clone()
            dec = sbecodec.decode_batch(d, o, sbecodec.DEC_PARSE_MESSAGE, out=sbecodec.alloc_decoded(n, "cuda"),
                                        in_bytes=data.size)
            return d, o, dec, sbecodec.extract_json(d, o, dec, paths), sbecodec.classify_commits(d, o, dec, table)
        R = Rot(make)
        torch.cuda.synchronize()
        dec0, got0 = R.sets[0][2], R.sets[0][3].numpy()
        pbytes = int(dec0.view_len[:n, 3].to(torch.int64).sum().item())
        found = (got0["kind"] != 0).sum(axis=0).tolist()

        def fn():
            d, o, dec, out, _ = R.next()
            sbecodec.extract_json(d, o, dec, paths, out=out)
        ms = _event_ms(fn, steps, warmup)

        def cfn():
            d, o, dec, _, plan = R.next()
            sbecodec.classify_commits(d, o, dec, table, out=plan)
        cms = _event_ms(cfn, steps, warmup)
        line(f"json_extract_{name}", n, ms * 1e-3,
             {"sbe_json_extract_batch (9 order-id paths)": (ms, pbytes + (18 + 2 + 9 * 9) * n),
              "sbe_classify_commits (same buffers, same run)": (cms, pbytes + 32 * n + (42 + 15) * n)})
        print(json.dumps({"row": f"json_extract_{name}", "payload_bytes": pbytes, "payload_GBps": pbytes / (ms * 1e-3) / 1e9,
                          "doc_counts": np.bincount(got0["doc"], minlength=5).tolist(), "found_per_path": found}), flush=True)
        del R
        torch.cuda.empty_cache()


def row_order_select(steps, warmup):
    """sbe_order_select after a parse_message decode of 1 M fixed-256 Orders: with CREATE_ORDER types
    (every record is decided by its type: no payload is staged or searched) and with an empty type
    and the nested payload of the json_extract row (every payload is searched; the needle lies 75
    bytes in).  Bytes: 46 B of descriptors (rec_off 8, status 1, flags 1, hdr 4, the offsets and
    lengths of views 0, 1 and 3 24) and 3 B of outputs a record, the type and topic read, and in
    the full-search case the payloads.  CPU, in the same row: the
    host loop the call replaces (ParsedBatch::result_into + the predicates per record,
    tests/select/select_baseline), one thread and CPU_THREADS threads."""
    import subprocess
    n = 1_000_000
    arena, L, ts = T.fixed256_orders(n)
    nested = (b'{"uuid":"cid_0123456789abcdefg","message":{"message":{"order_details":'
              b'{"client_order_id":"cid_0123456789abcdefg"}}}}')
    full = arena.reshape(n, 222).copy()
    full[:, 47:190] = np.frombuffer(nested.ljust(143), np.uint8)
    # an empty type: its 12 bytes go to the uuid, the record keeps its 256 bytes
    L_full = np.asarray(L, np.uint32).reshape(n, 5).copy()
    L_full[:, 1], L_full[:, 2] = 0, 41
    for which, (name, ar, ln) in enumerate((("skipped_search", arena, L), ("full_search", full.reshape(-1), L_full))):
        data, off = T.oracle_encode(ar, ln, ts)[:2]
        d0, o0 = dev(data, torch.uint8), dev(np.asarray(off, np.uint64), torch.int64)

        def make(k):
            d, o = d0.clone(), o0.clone()
            dec = sbecodec.decode_batch(d, o, sbecodec.DEC_PARSE_MESSAGE, out=sbecodec.alloc_decoded(n, "cuda"),
                                        in_bytes=data.size)
            return d, o, dec, sbecodec.order_select(d, o, dec)
        R = Rot(make)
        torch.cuda.synchronize()
        dec0, got0 = R.sets[0][2], R.sets[0][3].numpy()
        pbytes = int(dec0.view_len[:n, 3].to(torch.int64).sum().item()) if which else 0
        tbytes = int(dec0.view_len[:n, :2].to(torch.int64).sum().item())
        assert got0["totals"].tolist() == [n, n], got0["totals"]

        def fn():
            d, o, dec, out = R.next()
            sbecodec.order_select(d, o, dec, out=out)
        ms = _event_ms(fn, steps, warmup)
        extra = {"row": f"order_select_{name}", "payload_bytes": pbytes, "payload_GBps": pbytes / (ms * 1e-3) / 1e9,
                 "pred_counts": np.bincount(got0["pred"], minlength=16).tolist(),
                 "class_counts": np.bincount(got0["topic_class"], minlength=3).tolist()}
        if not NO_CPU:
            dd = os.path.join(ROOT, "tests", "select")
            subprocess.run(["make", "-s", "-C", dd, "select_baseline"], check=True)
            for th in (1, CPU_THREADS):
                cpu = json.loads(subprocess.run([os.path.join(dd, "select_baseline"), str(n), str(which), str(th)], check=True,
                                                capture_output=True, text=True).stdout)
                assert cpu["selected"] == n and cpu["record_bytes"] == 256, cpu
                extra[f"cpu_mask_loop_ms_{th}_threads"] = cpu["mask_loop_ms"]
            extra["cpu_over_device"] = extra[f"cpu_mask_loop_ms_{CPU_THREADS}_threads"] / ms
        print(json.dumps(extra), flush=True)
        line(f"order_select_{name}", n, ms * 1e-3,
             {"sbe_order_select (memset + 1 launch)": (ms, pbytes + tbytes + (46 + 3) * n)})
        del R
        torch.cuda.empty_cache()


def _term_block(total):
    """The block of the term_scan and term_poll rows, and its messages."""
    import termscan_lib as S
    data, off = T.mixed_records(60_000)
    b = S.Block()
    long_payload = bytes(32 + j % 90 for j in range(6000))
    nmsg = 0
    for i in range(60_000):
        rec = bytes(data[int(off[i]):int(off[i + 1])])
        if i % 64 == 63:
            rec = T.tm_wire((b"orders", b"CREATE_ORDER", b"msg_%025d" % i, long_payload, b"{}"), 1_760_000_000_000 + i)
        rec = T.session_wrap(rec)
        if len(b) + 32 * ((len(rec) + 1375) // 1376) + S.align(len(rec)) + 64 > total:
            break
        for k in range(0, len(rec), 1376):
            b.frame(rec[k: k + 1376], (S.BEGIN if k == 0 else 0) | (S.ENDF if k + 1376 >= len(rec) else 0))
        nmsg += 1
    b.pad_to(total)
    return b.bytes(), nmsg


def row_term_scan(steps, warmup):
    """sbe_term_scan over a raw 16 MiB term-buffer block: config-3 records, session-framed, one
    BEGIN|END frame each, with every 64th message a 6 KB TopicMessage in BEGIN / middle / END frames of
    at most 1376 payload bytes.  Timed in the same run: the scan alone (tables and payload copy), the
    scan with tables only, scan + sbe_reassemble_fragments, a device copy of the payload bytes (the
    ceiling), and on the host the mirror's one-thread term_walk alone and with its payload memcpy
    (tests/term/term_baseline)."""
    import subprocess
    import tempfile
    import termscan_lib as S
    total = 16 << 20
    blk, nmsg = _term_block(total)
    w = S.walk(blk)
    n, pbytes = w["fragments"], w["frag_off"][-1]
    d0 = torch.from_numpy(np.frombuffer(blk, np.uint8).copy()).cuda()
    ws = torch.empty(int(sbecodec.lib().sbe_term_scan_workspace_size(total)), dtype=torch.uint8, device="cuda")
    rws = torch.empty(int(sbecodec.lib().sbe_reassemble_workspace_size(n)), dtype=torch.uint8, device="cuda")
    R = Rot(lambda k: (d0.clone(), torch.empty(total, dtype=torch.uint8, device="cuda"),
                       torch.empty(total, dtype=torch.uint8, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda")))
    first = sbecodec.term_scan(d0, workspace=ws)
    torch.cuda.synchronize()
    c = first.counts.cpu().numpy()
    assert (int(c[0]), int(c[1]), int(c[2]), int(c[3])) == (n, total, pbytes, S.END), c
    assert first.out[:pbytes].cpu().numpy().tobytes() == w["payload"]

    def scan():
        d, out, _, _ = R.next()
        return sbecodec.term_scan(d, out=out, capacity=n + 1, workspace=ws)

    def tables():
        d, _, _, _ = R.next()
        sbecodec.term_scan(d, capacity=n + 1, want_out=False, workspace=ws)

    def chain():  # n: the fragment count a caller reads from counts[0] (here known from the first call)
        d, out, out2, mo = R.next()
        s = sbecodec.term_scan(d, out=out, capacity=n + 1, workspace=ws)
        sbecodec.reassemble(s.out, s.frag_off[: n + 1], s.flags[:n], out=out2, msg_off=mo, workspace=rws)

    def copy():
        d, out, _, _ = R.next()
        out[:pbytes].copy_(d[:pbytes])

    ms_scan, ms_tab, ms_chain, ms_copy = (_event_ms(f, steps, warmup) for f in (scan, tables, chain, copy))
    extra = {"row": "term_scan_detail", "block_bytes": total, "fragments": n, "messages": nmsg, "payload_bytes": pbytes,
             "scan_ms": ms_scan, "scan_tables_only_ms": ms_tab, "scan_reassemble_ms": ms_chain, "device_copy_ms": ms_copy,
             "launches": "term_tile_chain, term_walk_tiles, term_emit", "tile_bytes": sbecodec.term_scan_tile(),
             "tiles": total // sbecodec.term_scan_tile()}
    if not NO_CPU:
        dd = os.path.join(ROOT, "tests", "term")
        subprocess.run(["make", "-s", "-C", dd, "term_baseline"], check=True)
        with tempfile.NamedTemporaryFile(suffix=".bin") as tf:
            tf.write(blk)
            tf.flush()
            cpu = json.loads(subprocess.run([os.path.join(dd, "term_baseline"), tf.name], check=True, capture_output=True,
                                            text=True).stdout)
        assert cpu["fragments"] == n and cpu["payload_bytes"] == pbytes
        extra["host_term_walk_ms"] = cpu["term_walk_ms"]
        extra["host_term_walk_memcpy_ms"] = cpu["term_walk_memcpy_ms"]
        set_cpu(n / (cpu["term_walk_memcpy_ms"] * 1e-3), "the same block, host mirror term_walk + payload memcpy, 1 thread "
                "(sequential by definition)", cores=1)
    print(json.dumps(extra), flush=True)
    # the block's header sectors read twice (chain, emit), payload read and written, 12 B per slot
    # written and 12 B per tile entry read, the tables written
    line("term_scan", n, ms_scan * 1e-3, {"sbe_term_scan (3 launches)": (ms_scan, 2 * total + 2 * pbytes + 12 * (total // 32) + 13 * n)})


def row_term_poll(steps, warmup):
    """sbe_term_poll over the term_scan row's block (16 MiB, whole messages out in one call, no host
    read), and in the same run the path it replaces for a device-resident caller: sbe_term_scan with
    its payload copy, then sbe_reassemble_fragments with n known (the term_scan row's
    scan_reassemble_ms), measured twice, so the spread between two measurements of one thing is on
    record.  Device events over whole calls, rotated sets; the first call's counts, msg_off and every
    message byte are checked against the restatements before timing."""
    import termscan_lib as S
    total = 16 << 20
    blk, nmsg = _term_block(total)
    w = S.walk(blk)
    n, pbytes = w["fragments"], w["frag_off"][-1]
    msgs, carry = T.oracle_reassemble(np.frombuffer(w["payload"], np.uint8), np.array(w["frag_off"], np.uint64),
                                      np.array(w["flags"], np.uint8))
    assert len(msgs) == nmsg and carry == b""
    d0 = torch.from_numpy(np.frombuffer(blk, np.uint8).copy()).cuda()
    ws = torch.empty(int(sbecodec.lib().sbe_term_scan_workspace_size(total)), dtype=torch.uint8, device="cuda")
    rws = torch.empty(int(sbecodec.lib().sbe_reassemble_workspace_size(n)), dtype=torch.uint8, device="cuda")
    pws = torch.empty(int(sbecodec.lib().sbe_term_poll_workspace_size(total, n + 1)), dtype=torch.uint8, device="cuda")
    R = Rot(lambda k: (d0.clone(), torch.empty(total, dtype=torch.uint8, device="cuda"),
                       torch.empty(total, dtype=torch.uint8, device="cuda"), torch.empty(n + 2, dtype=torch.int64, device="cuda")))
    first = sbecodec.term_poll(d0, capacity=n + 1, workspace=pws)
    torch.cuda.synchronize()
    c = [int(x) for x in first.counts.cpu().numpy()]
    assert c == [n, total, pbytes, S.END, nmsg, 0], c
    mo = first.msg_off[: nmsg + 1].cpu().numpy()
    assert mo.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in msgs])]).tolist()
    assert first.out[: int(mo[-1])].cpu().numpy().tobytes() == b"".join(msgs)

    def poll():
        d, out, _, mo = R.next()
        sbecodec.term_poll(d, capacity=n + 1, out=out, msg_off=mo, workspace=pws)

    def chain():  # n: the fragment count a caller reads from counts[0] (here known from the first call)
        d, out, out2, mo = R.next()
        s = sbecodec.term_scan(d, out=out, capacity=n + 1, workspace=ws)
        sbecodec.reassemble(s.out, s.frag_off[: n + 1], s.flags[:n], out=out2, msg_off=mo, workspace=rws)

    ms_chain, ms_poll, ms_chain2 = (_event_ms(f, steps, warmup) for f in (chain, poll, chain))
    print(json.dumps({"row": "term_poll_detail", "block_bytes": total, "fragments": n, "messages": nmsg,
                      "payload_bytes": pbytes, "term_poll_ms": ms_poll, "scan_reassemble_ms": ms_chain,
                      "scan_reassemble_again_ms": ms_chain2, "spread_ms": abs(ms_chain - ms_chain2),
                      "launches": "term_tile_chain, term_walk_tiles, term_emit, tp_frag_reduce, tp_frag_scan_blocks, "
                                  "tp_frag_scan_msgs, term_poll_gather"}), flush=True)
    # the block's header sectors read twice (chain, emit), payload read and written once, 12 B per
    # slot written and 12 B per tile entry read, the fragment tables written and read by the scans
    line("term_poll", n, ms_poll * 1e-3, {"sbe_term_poll (7 launches)": (ms_poll, 2 * total + 2 * pbytes + 12 * (total // 32) + 3 * 13 * n)})


def row_term_append(steps, warmup):
    """sbe_term_append of the records of the term_scan row (config-3 records, session-framed, every
    64th a 6 KB TopicMessage) into a 16 MiB term-buffer block at MTU 1408: the records lie encoded in
    device memory first, the frames are built on the device.  Timed in the same run: the append, a
    device copy of the same payload bytes (the ceiling), and on the host the mirror's one-thread
    term_append (tests/termappend/term_append_baseline)."""
    import subprocess
    import tempfile
    import termappend_lib as A
    total, mtu = 16 << 20, 1408
    data, off = T.mixed_records(60_000)
    long_payload = bytes(32 + j % 90 for j in range(6000))
    recs, used = [], 0
    for i in range(60_000):
        rec = bytes(data[int(off[i]):int(off[i + 1])])
        if i % 64 == 63:
            rec = T.tm_wire((b"orders", b"CREATE_ORDER", b"msg_%025d" % i, long_payload, b"{}"), 1_760_000_000_000 + i)
        rec = T.session_wrap(rec)
        if used + A.required(len(rec), mtu) + 64 > total:
            break
        used += A.required(len(rec), mtu)
        recs.append(rec)
    n = len(recs)
    payload, roff = A.pack(recs)
    pbytes = len(payload)
    exp = A.append(bytes(total), 0, recs, mtu=mtu, max_message_length=total // 8)
    assert (exp["appended"], exp["next"], exp["stop"]) == (n, used, A.END)
    d0 = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).cuda()
    o0 = torch.from_numpy(np.asarray(roff, np.int64)).cuda()
    ws = torch.empty(int(sbecodec.lib().sbe_term_append_workspace_size(n)), dtype=torch.uint8, device="cuda")
    hdr = sbecodec.TermHeader(7, 1001, 3, 0, 1)
    R = Rot(lambda k: (d0.clone(), o0.clone(), torch.zeros(total, dtype=torch.uint8, device="cuda"),
                       torch.empty(n, dtype=torch.int64, device="cuda")))
    first = sbecodec.term_append(R.sets[0][2], d0, o0, mtu=mtu, header=hdr, workspace=ws)
    torch.cuda.synchronize()
    c = first.counts.cpu().numpy()
    assert (int(c[0]), int(c[1]), int(c[2]), int(c[3])) == (n, used, pbytes, A.END), c
    assert first.block[:used].cpu().numpy().tobytes() == exp["block"][:used]
    assert first.rec_tail.cpu().numpy().tolist() == exp["rec_tail"]

    def append():
        d, o, blk, tails = R.next()
        sbecodec.term_append(blk, d, o, mtu=mtu, header=hdr, workspace=ws, rec_tail=tails)

    def copy():
        d, _, blk, _ = R.next()
        blk[:pbytes].copy_(d)

    ms_app, ms_copy = (_event_ms(f, steps, warmup) for f in (append, copy))
    # the payload read, [start, next) written, rec_off read by three of the launches, the tails written and read
    nbytes = pbytes + used + 3 * 8 * (n + 1) + 2 * 8 * n
    extra = {"row": "term_append_detail", "block_bytes": total, "records": n, "payload_bytes": pbytes, "written_bytes": used,
             "frames": sum(max(1, -(-len(r) // (mtu - 32))) for r in recs), "append_ms": ms_app, "device_copy_ms": ms_copy,
             "counted_bytes": nbytes, "append_GBps": nbytes / (ms_app * 1e-3) / 1e9,
             "copy_GBps": 2 * pbytes / (ms_copy * 1e-3) / 1e9,
             "launches": "ta_sums, ta_scan_blocks, ta_tails, ta_write", "tile_bytes": sbecodec.term_append_tile(),
             "tiles": -(-used // sbecodec.term_append_tile())}
    if not NO_CPU:
        dd = os.path.join(ROOT, "tests", "termappend")
        subprocess.run(["make", "-s", "-C", dd, "term_append_baseline"], check=True)
        with tempfile.NamedTemporaryFile(suffix=".bin") as tf:
            tf.write(np.asarray([n] + roff, np.uint64).tobytes())
            tf.write(payload)
            tf.flush()
            cpu = json.loads(subprocess.run([os.path.join(dd, "term_append_baseline"), tf.name, str(total)], check=True,
                                            capture_output=True, text=True).stdout)
        assert (cpu["appended"], cpu["next"], cpu["stop"]) == (n, used, A.END), cpu
        extra["host_term_append_ms"] = cpu["term_append_ms"]
        extra["host_over_device"] = cpu["term_append_ms"] / ms_app
        set_cpu(n / (cpu["term_append_ms"] * 1e-3), "the same records, host mirror term_append, 1 thread (one publication "
                "appends serially)", cores=1)
    print(json.dumps(extra), flush=True)
    line("term_append", n, ms_app * 1e-3, {"sbe_term_append (4 launches)": (ms_app, nbytes)})


def _wall_ms(fn, steps, warmup):
    """Wall clock per call, the stream drained at both ends: for paths whose host reads are part of the cost."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def row_egress_step(steps, warmup):
    """The subscriber's egress step on a raw 16 MiB term-buffer block of session-framed fixed-256
    Orders (one BEGIN|END frame each, every header naming a known topic, so every message commits):
    term poll, decode, classify, emit, term append of the commit frames into an ingress block.
    Counted: egress_commit_step, one enqueue, the message count and the frame count staying on the
    device.  Staged (the baseline, the path before the counted calls): the same kernels through the
    uncounted calls, the host reading counts[4] before the decode and totals[0] before it builds the
    frame table (two device ops) for the append.  Both in one process on the same rotated inputs,
    wall clock per step with the stream drained at the end of the timed loop, the staged form measured
    again behind the counted one.  Then, on 1 M fixed-256 records: sbe_decode_batch_counted at count ==
    capacity against sbe_decode_batch_sized at that n, and at count == capacity / 16 against the sized
    call at that n (what the empty tail of the grid costs), device events."""
    import termscan_lib as S
    total = 16 << 20
    per = 32 + 32 + 256
    nmsg = (total - 64) // per
    arena, L, ts = T.fixed256_orders(nmsg)
    a2 = arena.reshape(nmsg, 222).copy()
    a2[:, 190:] = np.frombuffer(b'{"topic":"orders","a":"CREATE"} ', np.uint8)
    data, off = T.oracle_encode_session(a2.reshape(-1), L, ts, 7, 9)[:2]
    assert int(off[nmsg]) == nmsg * 288
    b = S.Block()
    for i in range(nmsg):
        b.frame(bytes(data[288 * i: 288 * (i + 1)]), S.BEGIN | S.ENDF)
    b.pad_to(total)
    blk = b.bytes()
    topics = [b"orders", b"order_request_topic", b"order_notification_topic"]
    idents = [b"client-01", b"sub-req", b"sub-ntf"]
    table = sbecodec.commit_topic_table(topics, "cuda")
    itab = sbecodec.commit_identifier_table(idents, "cuda")
    tid = dev(np.array([3, 1, 2], np.uint32), torch.int32)
    d0 = torch.from_numpy(np.frombuffer(blk, np.uint8).copy()).cuda()
    cap = nmsg + 1
    kw = dict(leadership_term_id=7, cluster_session_id=9)
    ing_bytes = 32 << 20

    def make(k):
        d = d0.clone()
        ing = torch.empty(ing_bytes, dtype=torch.uint8, device="cuda")
        s = sbecodec.egress_commit_step(d, 0, None, table, tid, idents, ing, capacity=cap, avg_record_bytes=288, **kw)
        return d, ing, s

    R = Rot(make)
    torch.cuda.synchronize()
    s0 = R.sets[0][2]
    assert int(s0.polled.counts[4]) == nmsg and int(s0.frames.totals[0]) == nmsg
    assert int(s0.appended.counts[0]) == nmsg and int(s0.appended.counts[3]) == sbecodec.TERM_APPEND_END
    pws = torch.empty(int(sbecodec.lib().sbe_term_poll_workspace_size(total, cap)), dtype=torch.uint8, device="cuda")

    def counted():
        d, ing, s = R.next()
        sbecodec.egress_commit_step(d, 0, None, table, tid, itab, ing, capacity=cap, avg_record_bytes=288, bufs=s, **kw)

    def staged():
        d, ing, s = R.next()
        p = sbecodec.term_poll(d, capacity=cap, out=s.polled.out, msg_off=s.polled.msg_off, counts=s.polled.counts, workspace=pws)
        m = int(p.counts[4])  # host read 1
        ro = p.msg_off[: m + 1]
        dec = sbecodec.decode_batch(p.out, ro, sbecodec.DEC_PARSE_MESSAGE, out=s.decoded, seq=s.decoded.seq, in_bytes=288 * m)
        plan = sbecodec.classify_commits(p.out, ro, dec, table, out=s.plan)
        f = s.frames
        fr = sbecodec.emit_commit_offsets(p.out, ro, dec, plan, tid, itab, out=f.out, out_off=f.out_off, status=f.status,
                                          emit_idx=f.emit_idx, totals=f.totals, workspace=f.workspace, **kw)
        t0 = int(fr.totals[0])  # host read 2, then the frame table: the frames lie back to back in record order
        tab = torch.cat([fr.out_off[fr.emit_idx[:t0]], fr.out_off[m: m + 1]])
        sbecodec.term_append(ing, fr.out, tab, rec_tail=s.appended.rec_tail, counts=s.appended.counts)

    staged()
    torch.cuda.synchronize()
    ref = R.sets[0]
    x = sbecodec.egress_commit_step(ref[0], 0, None, table, tid, idents, torch.empty_like(ref[1]), capacity=cap, **kw)
    staged_ing = R.sets[(R.k - 1) % len(R.sets)][1]
    torch.cuda.synchronize()
    end = int(x.appended.counts[1])
    assert torch.equal(x.appended.block[:end], staged_ing[:end])  # the two forms write the same ingress bytes
    ms_s = _wall_ms(staged, steps, warmup)
    ms_c = _wall_ms(counted, steps, warmup)
    ms_s2 = _wall_ms(staged, steps, warmup)
    ev_c = _event_ms(counted, steps, warmup)
    print(json.dumps({"row": "egress_step_detail", "block_bytes": total, "messages": nmsg, "frames": nmsg,
                      "ingress_bytes": end, "counted_wall_ms": ms_c, "staged_wall_ms": ms_s, "staged_wall_again_ms": ms_s2,
                      "counted_event_ms": ev_c, "staged_over_counted": ms_s / ms_c}), flush=True)
    del R, s0, x, ref
    torch.cuda.empty_cache()

    # the counted decode beside the sized one
    n = 1_000_000
    arena, L, ts = T.fixed256_orders(n)
    data, off = T.oracle_encode(arena, L, ts)[:2]
    dd, oo = dev(data, torch.uint8), dev(np.asarray(off, np.uint64), torch.int64)
    R2 = Rot(lambda k: (dd.clone(), oo.clone(), sbecodec.alloc_decoded(n, "cuda")))
    full, part = torch.full((1,), n, dtype=torch.int64, device="cuda"), torch.full((1,), n // 16, dtype=torch.int64, device="cuda")

    def sized(m):
        def fn():
            d, o, out = R2.next()
            sbecodec.decode_batch(d, o[: m + 1], sbecodec.DEC_PARSE_MESSAGE, out=out, in_bytes=256 * m)
        return fn

    def counted_dec(cnt):
        def fn():
            d, o, out = R2.next()
            sbecodec.decode_batch_counted(d, o, cnt, n, sbecodec.DEC_PARSE_MESSAGE, out=out, avg_record_bytes=256)
        return fn

    ms = {k: _event_ms(f, steps, warmup) for k, f in (("sized_full", sized(n)), ("counted_full", counted_dec(full)),
                                                      ("sized_full_again", sized(n)), ("sized_sixteenth", sized(n // 16)),
                                                      ("counted_sixteenth", counted_dec(part)),
                                                      ("sized_sixteenth_again", sized(n // 16)))}
    print(json.dumps({"row": "decode_counted_detail", "capacity": n, **{k + "_ms": v for k, v in ms.items()}}), flush=True)
    line("egress_step", nmsg, ms_c * 1e-3,
         {"egress_commit_step (one enqueue, wall clock)": (ms_c, 2 * total + nmsg * (288 + DESC) + 2 * end),
          "staged: the uncounted calls with two host reads (wall clock)": (ms_s, 2 * total + nmsg * (288 + DESC) + 2 * end)})


def row_commit_emit(steps, warmup):
    """sbe_emit_commit_offsets over 1 M decoded and classified fixed-256 Orders whose headers all
    carry a known topic (every record emits a session-framed CommitOffsetLite; short identifiers),
    and, in the same run, the device part of the chain it replaces: sbe_encode_lite_batch (301) on
    a pre-gathered arena of the same ids and identifiers.  The baseline's host gather and its
    session framing are left out, which favours the baseline.  Bytes of the fused call, per record:
    rec_off 8, cm 1, topic_idx 4, status + flags 2, view 2 offset and length 8, seq 8 and the id
    read; out_off 8, status 1, emit_idx 8 and the frame written.  The baseline's: lengths 8,
    topicId 4, sequence 8 and both strings read; out_off 8, status 1 and the bare record written."""
    n = 1_000_000
    arena, L, ts = T.fixed256_orders(n)
    a2 = arena.reshape(n, 222).copy()
    a2[:, 190:] = np.frombuffer(b'{"topic":"orders","a":"CREATE"} ', np.uint8)
    data, off = T.oracle_encode(a2.reshape(-1), L, ts)[:2]
    topics = [b"orders", b"order_request_topic", b"order_notification_topic"]
    idents = [b"client-01", b"sub-req", b"sub-ntf"]
    d0, o0 = dev(data, torch.uint8), dev(np.asarray(off, np.uint64), torch.int64)
    table = sbecodec.commit_topic_table(topics, "cuda")
    itab = sbecodec.commit_identifier_table(idents, "cuda")
    tid = dev(np.array([3, 1, 2], np.uint32), torch.int32)
    # the baseline's arena, gathered on the host once: id and identifier of every record, back to back
    Lh = np.asarray(L, np.int64).reshape(n, 5)
    id_off = np.asarray(off[:-1], np.int64) + 24 + 2 + Lh[:, 0] + 2 + Lh[:, 1] + 2
    idl = Lh[:, 2]
    assert int(idl.min()) == int(idl.max())  # fixed-size records: one id length
    w = int(idl[0])
    ids = data[(id_off[:, None] + np.arange(w)[None, :]).reshape(-1)].reshape(n, w)
    g_arena = np.concatenate([ids, np.tile(np.frombuffer(idents[0], np.uint8), (n, 1))], axis=1).reshape(-1)
    g_len = np.tile(np.array([w, len(idents[0])], np.int32), n)
    g0 = (dev(g_arena, torch.uint8), dev(g_len, torch.int32), torch.full((n,), 3, dtype=torch.int32, device="cuda"),
          torch.zeros(n, dtype=torch.int64, device="cuda"))

    def make(k):
        d, o = d0.clone(), o0.clone()
        dec = sbecodec.decode_batch(d, o, sbecodec.DEC_PARSE_MESSAGE, out=sbecodec.alloc_decoded(n, "cuda"),
                                    in_bytes=data.size, seq=True)
        plan = sbecodec.classify_commits(d, o, dec, table)
        fr = sbecodec.emit_commit_offsets(d, o, dec, plan, tid, itab, leadership_term_id=7, cluster_session_id=9)
        g = tuple(x.clone() for x in g0)
        enc = sbecodec.encode_lite_batch(sbecodec.COMMIT_OFFSET_LITE, *g)
        return d, o, dec, plan, fr, g, enc

    R = Rot(make)
    torch.cuda.synchronize()
    d, o, dec, plan, fr0, _, enc0 = R.sets[0]
    assert int(fr0.totals[0]) == n and int(fr0.status.min()) == sbecodec.CE_EMITTED
    bare = sbecodec.emit_commit_offsets(d, o, dec, plan, tid, itab, session=False)
    torch.cuda.synchronize()
    total_b = int(enc0.out_off[n])
    # without the session frame the fused call writes the baseline's stream
    assert int(bare.totals[1]) == total_b and torch.equal(bare.out[:total_b], enc0.out[:total_b])
    del bare
    total = int(fr0.totals[1])

    def fused_fn():
        d, o, dec, plan, fr, _, _ = R.next()
        sbecodec.emit_commit_offsets(d, o, dec, plan, tid, itab, leadership_term_id=7, cluster_session_id=9,
                                     out=fr.out, out_off=fr.out_off, status=fr.status, emit_idx=fr.emit_idx,
                                     totals=fr.totals, workspace=fr.workspace)

    def base_fn():
        *_, g, enc = R.next()
        sbecodec.encode_lite_batch(sbecodec.COMMIT_OFFSET_LITE, *g, out=enc.out, out_off=enc.out_off,
                                   status=enc.status, workspace=enc.workspace)

    ms_f = _event_ms(fused_fn, steps, warmup)
    ms_b = _event_ms(base_fn, steps, warmup)
    ms_f2 = _event_ms(fused_fn, steps, warmup)  # again after the baseline: drift between the two shows here
    nb_f = n * (8 + 1 + 4 + 2 + 8 + 8 + w) + n * (8 + 1 + 8) + total
    nb_b = n * (8 + 4 + 8 + w + len(idents[0])) + n * (8 + 1) + total_b
    if max(ms_f, ms_f2) > ms_b:
        print(f"WARNING commit_emit: fused {ms_f:.4f} / {ms_f2:.4f} ms is slower than the partial baseline {ms_b:.4f} ms",
              file=sys.stderr, flush=True)
    print(json.dumps({"row": "commit_emit", "fused_not_slower_than_partial_baseline": bool(max(ms_f, ms_f2) <= ms_b),
                      "baseline_over_fused": ms_b / ms_f, "id_bytes": w, "frame_bytes": total // n}), flush=True)
    line("commit_emit", n, ms_f * 1e-3,
         {"sbe_emit_commit_offsets (fused, session-framed: all launches)": (ms_f, nb_f),
          "sbe_emit_commit_offsets (measured again after the baseline)": (ms_f2, nb_f),
          "baseline: sbe_encode_lite_batch on a pre-gathered arena (no gather, no session frame)": (ms_b, nb_b)})


def row_commit_fallback(steps, warmup):
    """sbe_emit_commit_offsets_ex with a fallback over the commit_emit batch (1 M decoded and
    classified fixed-256 Orders, every header's topic a table entry) and a table in which every
    entry has id 0: every record emits the session-framed JSON TopicMessage.  Bytes per record, as
    the commit_emit row counts them: rec_off 8, cm 1, topic_idx 4, status + flags 2, view 2 offset
    and length 8, seq 8, ts 8 and the id read; out_off 8, status 1, emit_idx 8 and the frame
    written."""
    n = 1_000_000
    arena, L, ts = T.fixed256_orders(n)
    a2 = arena.reshape(n, 222).copy()
    a2[:, 190:] = np.frombuffer(b'{"topic":"orders","a":"CREATE"} ', np.uint8)
    data, off = T.oracle_encode(a2.reshape(-1), L, ts)[:2]
    topics = [b"orders", b"order_request_topic", b"order_notification_topic"]
    idents = [b"client-01", b"sub-req", b"sub-ntf"]
    d0, o0 = dev(data, torch.uint8), dev(np.asarray(off, np.uint64), torch.int64)
    table = sbecodec.commit_topic_table(topics, "cuda")
    itab = sbecodec.commit_identifier_table(idents, "cuda")
    tid = dev(np.zeros(3, np.uint32), torch.int32)
    fb = sbecodec.CommitFallback(table, b"client-01", 1_700_000_000_123_456_789, 1_700_000_000_223_456_789)
    w = int(np.asarray(L).reshape(n, 5)[0, 2])

    def make(k):
        d, o = d0.clone(), o0.clone()
        dec = sbecodec.decode_batch(d, o, sbecodec.DEC_PARSE_MESSAGE, out=sbecodec.alloc_decoded(n, "cuda"),
                                    in_bytes=data.size, seq=True)
        plan = sbecodec.classify_commits(d, o, dec, table)
        sized = sbecodec.emit_commit_offsets(d, o, dec, plan, tid, itab, leadership_term_id=7, cluster_session_id=9,
                                             out=None, out_capacity=0, fallback=fb)
        torch.cuda.synchronize()
        fr = sbecodec.emit_commit_offsets(d, o, dec, plan, tid, itab, leadership_term_id=7, cluster_session_id=9,
                                          out_capacity=int(sized.totals[1]), out_off=sized.out_off, status=sized.status,
                                          emit_idx=sized.emit_idx, totals=sized.totals, workspace=sized.workspace,
                                          fallback=fb)
        return d, o, dec, plan, fr

    R = Rot(make)
    torch.cuda.synchronize()
    fr0 = R.sets[0][4]
    assert int(fr0.totals[0]) == n and int(fr0.status.min()) == int(fr0.status.max()) == sbecodec.CE_EMITTED_JSON
    total = int(fr0.totals[1])

    def fn():
        d, o, dec, plan, fr = R.next()
        sbecodec.emit_commit_offsets(d, o, dec, plan, tid, itab, leadership_term_id=7, cluster_session_id=9,
                                     out=fr.out, out_off=fr.out_off, status=fr.status, emit_idx=fr.emit_idx,
                                     totals=fr.totals, workspace=fr.workspace, fallback=fb)

    ms = _event_ms(fn, steps, warmup)
    nb = n * (8 + 1 + 4 + 2 + 8 + 8 + 8 + w) + n * (8 + 1 + 8) + total
    print(json.dumps({"row": "commit_fallback", "id_bytes": w, "frame_bytes": total // n}), flush=True)
    line("commit_fallback", n, ms * 1e-3,
         {"sbe_emit_commit_offsets_ex (fallback, every record a session-framed JSON frame: all launches)": (ms, nb)})


def row_ack_correlate(steps, warmup):
    """sbe_inflight_remember of 1 M publish_topic uuids into an empty 2 M-slot table, then
    sbe_inflight_match_acks of 1 M full acks (T.ack_wire; about 10 % ids nobody sent, 1 % ids that
    appeared earlier in the batch), with sbe_decode_batch(ON_EGRESS) of the same ack buffers timed in
    the same run.  Every step starts from an empty table (sbe_inflight_init, not timed).  Bytes,
    per record: remember reads the key (23), offset, length and ts (16), writes a status and a
    workspace word twice (9) and reads and writes one 64-B slot twice (launch A probes it, launch B
    fills it); match reads the id (23) and 25 B of descriptors, writes code and base_ns (9), the
    workspace word twice (8) and reads one slot twice.  The slot accesses are random 64-B lines: the
    row is latency-bound and these fractions of the HBM peak say how far from a stream it is.
    CPU: tests/inflight/map_baseline, one thread, the same emplace / find / erase sequence."""
    import subprocess
    n, cap = 1_000_000, 1 << 21
    rng = np.random.default_rng(0x5EED09)
    base = 1_760_000_000_000_000_000
    nanos = base + np.cumsum(rng.integers(1, 2000, n)).astype(np.int64)
    keys = np.frombuffer(b"".join(b"pub_%d" % v for v in nanos), np.uint8)
    assert keys.size == 23 * n
    key_off = (23 * np.arange(n)).astype(np.int32)
    key_len = np.full(n, 23, np.int32)
    send_ts = nanos.copy()
    # the acks: a shuffled 89 % of the sent ids, 10 % strangers, 1 % repeats of an earlier ack of the batch
    kind = rng.random(n)
    ids = nanos[rng.permutation(n)]
    strangers = kind < 0.10
    ids[strangers] = base - 1 - rng.integers(0, 10 ** 9, int(strangers.sum()))
    rep = np.nonzero(kind > 0.99)[0]
    rep = rep[rep > 0]
    ids[rep] = ids[(rep * rng.random(rep.size)).astype(np.int64)]
    recs = [T.ack_wire(b"pub_%d" % v, b"orders", b"c", base + 5) + b"\0" * 8 for v in ids]  # len - 8: see ack_decoder.cpp:67
    data, off = T.pack_records(recs)
    k0, o0, l0, t0 = dev(keys, torch.uint8), dev(key_off, torch.int32), dev(key_len, torch.int32), dev(send_ts, torch.int64)
    d0, r0 = dev(data, torch.uint8), dev(off, torch.int64)

    def make(k):
        tbl = sbecodec.Inflight(cap, "cuda")
        d, r = d0.clone(), r0.clone()
        dec = sbecodec.decode_batch(d, r, sbecodec.DEC_ON_EGRESS, out=sbecodec.alloc_decoded(n, "cuda"), in_bytes=data.size)
        st = tbl.remember(k0, o0, l0, t0)
        res = tbl.match_acks(d, r, dec)
        return tbl, k0.clone(), o0.clone(), l0.clone(), t0.clone(), d, r, dec, st, res
    R = Rot(make)
    torch.cuda.synchronize()
    st0, res0 = R.sets[0][8], R.sets[0][9].numpy()
    assert int(st0.max()) == sbecodec.INF_INSERTED  # nanos are strictly increasing: no duplicate key
    codes = np.bincount(res0["code"], minlength=4).tolist()
    # the model: a dict over the same sequence
    sent = dict(zip(nanos.tolist(), send_ts.tolist()))
    exp = np.array([sbecodec.ACK_MATCHED if sent.pop(v, None) is not None else sbecodec.ACK_UNMATCHED for v in ids.tolist()])
    assert np.array_equal(res0["code"], exp) and codes[1] == int(res0["counts"][0])

    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(steps)]
    def step(e):
        tbl, k, o, l, t, d, r, dec, st, res = R.next()
        tbl.clear()
        if e:
            e[0].record()
        tbl.remember(k, o, l, t, status=st)
        if e:
            e[1].record()
        sbecodec.decode_batch(d, r, sbecodec.DEC_ON_EGRESS, out=dec, in_bytes=data.size)
        if e:
            e[2].record()
        tbl.match_acks(d, r, dec, out=res)
        if e:
            e[3].record()
    for _ in range(warmup):
        step(None)
    torch.cuda.synchronize()
    for e in ev:
        step(e)
    torch.cuda.synchronize()
    t = np.array([[e[j].elapsed_time(e[j + 1]) for j in range(3)] for e in ev])
    ms_rem, ms_dec, ms_match = (float(v) for v in np.median(t, axis=0))
    kernels = {"sbe_inflight_remember (2 launches)": (ms_rem, (23 + 16 + 9 + 4 * 64) * n),
               "sbe_inflight_match_acks (memset + 2 launches)": (ms_match, (23 + 25 + 9 + 8 + 2 * 64) * n),
               "sbe_decode_batch ON_EGRESS (same ack buffers, same run)": (ms_dec, int(off[-1]) + 8 * n + DESC * n)}
    extra = {"row": "ack_correlate", "codes_none_matched_unmatched_long": codes, "capacity": cap,
             "ms_min": {"remember": float(t[:, 0].min()), "decode": float(t[:, 1].min()), "match": float(t[:, 2].min())},
             "match_over_decode": ms_match / ms_dec}
    if not NO_CPU:
        d = os.path.join(ROOT, "tests", "inflight")
        subprocess.run(["make", "-s", "-C", d, "map_baseline"], check=True)
        extra["cpu_unordered_map_one_thread"] = json.loads(subprocess.run([os.path.join(d, "map_baseline"), str(n)], check=True,
                                                                           capture_output=True, text=True).stdout)
    print(json.dumps(extra), flush=True)
    line("ack_correlate", n, (ms_rem + ms_match) * 1e-3, kernels)


def row_delivery_track(steps, warmup):
    """The second half of the subscriber's callback (examples/pubsub_reconnect_test.cpp:625-691) for
    1 M decoded fixed-256 Orders whose payloads carry message.message.client_order_id / order_id;
    about 10 % of the records repeat an earlier record of the batch.  Every step starts from empty
    message-id and client-id tables and a sent table refilled with the 1 M client ids (not timed).
    Timed as one region: sbe_delivery_keys + sbe_inflight_note_keys twice + sbe_inflight_lookup_keys
    (7 launches, 3 memsets); beside it the sbe_json_extract_batch the keys are made from.  Bytes, per
    record: keys reads 2 + 18 descriptor bytes and 2 + 9 * 9 of the extract and writes 40; each
    table pass reads a position, a length and the key (12 + 29 or 21), writes its results and the
    workspace word twice (5 or 9, 8) and touches one 64-B slot twice.  The slot accesses are random
    64-B lines, as in ack_correlate.  CPU: tests/delivery/set_baseline, one thread."""
    import subprocess
    n, cap = 1_000_000, 1 << 21
    arena, L, ts = T.fixed256_orders(n)
    rows = arena.reshape(n, 222).copy()
    shell = b'{"message":{"message":{"client_order_id":"cid_#################","order_id":"oid_#################"}}}'
    assert len(shell) <= 143
    pay = np.tile(np.frombuffer(shell.ljust(143), np.uint8), (n, 1))
    hol = [i for i, c in enumerate(shell) if c == ord("#")]
    cid_digits = rows[:, 47:190][:, [i for i, c in enumerate(T._PAYLOAD_T) if c == ord("#")][20:]]
    pay[:, hol[:17]] = cid_digits
    pay[:, hol[17:]] = cid_digits
    rows[:, 47:190] = pay
    sent_keys = np.ascontiguousarray(rows[:, 47 + hol[0] - 4: 47 + hol[0] + 17]).reshape(-1)  # "cid_" + 17 digits
    rng = np.random.default_rng(0x5EED0F9)
    again = np.nonzero(rng.random(n) < 0.10)[0]
    again = again[again > 0]
    src = (again * rng.random(again.size)).astype(np.int64)
    for i, j in zip(again.tolist(), src.tolist()):  # in order: a copy of a copy carries the first one's ids
        rows[i] = rows[j]
    data, off = T.oracle_encode(rows.reshape(-1), L, ts)[:2]
    paths = sbecodec.json_path_table(sbecodec.ORDER_ID_PATHS)
    d0, o0 = dev(data, torch.uint8), dev(np.asarray(off, np.uint64), torch.int64)
    k0 = dev(sent_keys, torch.uint8)
    ko0, kl0 = dev((21 * np.arange(n)).astype(np.int32), torch.int32), dev(np.full(n, 21, np.int32), torch.int32)

    def make(k):
        d, o = d0.clone(), o0.clone()
        dec = sbecodec.decode_batch(d, o, sbecodec.DEC_PARSE_MESSAGE, out=sbecodec.alloc_decoded(n, "cuda"), in_bytes=data.size)
        ids = sbecodec.extract_json(d, o, dec, paths)
        keys = sbecodec.delivery_keys(o, dec, ids)
        tabs = [sbecodec.Inflight(cap, "cuda") for _ in range(3)]
        tabs[2].remember(k0, ko0, kl0, ts_default=1000)
        res = (tabs[0].note_keys(d, keys.msg_pos, keys.msg_len), tabs[1].note_keys(d, keys.coid_pos, keys.coid_len),
               tabs[2].lookup_keys(d, keys.coid_pos, keys.coid_len))
        return d, o, dec, ids, keys, tabs, res
    R = Rot(make)
    torch.cuda.synchronize()
    keys0, res0 = R.sets[0][4].numpy(), [r.numpy() for r in R.sets[0][6]]
    # the model: a record is a redelivery exactly when it is a copy, and client ids are distinct
    assert np.unique(sent_keys.view("S21")).size == n
    is_again = np.zeros(n, bool)
    is_again[again] = True
    assert list(keys0["totals"]) == [n, 0] and (keys0["msg_len"] == 29).all() and (keys0["coid_len"] == 21).all()
    assert np.array_equal(res0[0]["code"] == sbecodec.DLV_AGAIN, is_again) and list(res0[0]["totals"]) == [n - again.size, again.size]
    assert np.array_equal(res0[1]["code"], res0[0]["code"])
    assert np.array_equal(res0[2]["code"] == sbecodec.SENT_REPEAT, is_again) and list(res0[2]["totals"]) == [n - again.size, again.size, 0]
    assert (res0[2]["value"][~is_again] == 1000).all()

    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(steps)]

    def step(e):
        d, o, dec, ids, keys, tabs, res = R.next()
        for t in tabs:
            t.clear()
        tabs[2].remember(k0, ko0, kl0, ts_default=1000)
        if e:
            e[0].record()
        sbecodec.extract_json(d, o, dec, paths, out=ids)
        if e:
            e[1].record()
        sbecodec.delivery_keys(o, dec, ids, out=keys)
        if e:
            e[2].record()
        tabs[0].note_keys(d, keys.msg_pos, keys.msg_len, code=res[0].code, count=res[0].count, totals=res[0].totals)
        tabs[1].note_keys(d, keys.coid_pos, keys.coid_len, code=res[1].code, count=res[1].count, totals=res[1].totals)
        tabs[2].lookup_keys(d, keys.coid_pos, keys.coid_len, code=res[2].code, value=res[2].value, totals=res[2].totals)
        if e:
            e[3].record()
    for _ in range(warmup):
        step(None)
    torch.cuda.synchronize()
    for e in ev:
        step(e)
    torch.cuda.synchronize()
    t = np.array([[e[j].elapsed_time(e[j + 1]) for j in range(3)] for e in ev])
    ms_ext, ms_keys, ms_tab = (float(v) for v in np.median(t, axis=0))
    pbytes = 143 * n
    kernels = {"sbe_delivery_keys (memset + 1 launch)": (ms_keys, (8 + 2 + 16 + 2 + 9 * 9 + 40) * n),
               "note, note, lookup (3 memsets + 6 launches)": (ms_tab, (2 * (12 + 29 + 5 + 8) + (12 + 21) * 2 + 5 + 9 + 16 + 6 * 64) * n),
               "sbe_json_extract_batch (9 order-id paths, same run)": (ms_ext, pbytes + (18 + 2 + 9 * 9) * n)}
    extra = {"row": "delivery_track", "redeliveries": int(again.size), "capacity": cap,
             "ms_min": {"extract": float(t[:, 0].min()), "keys": float(t[:, 1].min()), "tables": float(t[:, 2].min())},
             "track_over_extract": (ms_keys + ms_tab) / ms_ext}
    if not NO_CPU:
        d = os.path.join(ROOT, "tests", "delivery")
        subprocess.run(["make", "-s", "-C", d, "set_baseline"], check=True)
        extra["cpu_set_map_one_thread"] = json.loads(subprocess.run([os.path.join(d, "set_baseline"), str(n)], check=True,
                                                                    capture_output=True, text=True).stdout)
    print(json.dumps(extra), flush=True)
    line("delivery_track", n, (ms_keys + ms_tab) * 1e-3, kernels)


def row_delivery_report(steps, warmup):
    """The example's three reports (examples/pubsub_reconnect_test.cpp:130-204, :276-353) read on the
    device: 2 M-slot sent and received tables with 1 M sent "cid_<17 digits>" ids, about 1 % of them
    never received and about 1 % of the received ids never sent, and a log of 1 M latencies.  Timed
    as one region: sbe_inflight_list_keys sent \\ received and received \\ sent with limit 10
    (2 launches each), sbe_latency_report with the seven reference percentiles and `order`
    (a memset and 25 launches).  Nothing is modified, so the steps only rotate over the copies.
    Bytes: list_keys reads 64 B x capacity of `table` and one 64-B probe line in `other` per live
    entry that reaches the membership stage; the sort moves 16 B x count read and written per pass,
    over 8 passes.  CPU: tests/report/report_baseline, one thread."""
    import subprocess
    import report_lib as RL
    n, cap, log_cap = 1_000_000, 1 << 21, 1 << 20
    rng = np.random.default_rng(0x5EED0FA)

    def ids(prefix, count):
        k = np.empty((count, 21), np.uint8)
        k[:, :4] = np.frombuffer(prefix, np.uint8)
        k[:, 4:] = rng.integers(0, 10, (count, 17)) + ord("0")
        return k
    sent = ids(b"cid_", n)
    assert np.unique(sent.view("S21")).size == n
    got = rng.random(n) >= 0.01
    extra = ids(b"xid_", n // 100)
    recv = np.concatenate([sent[got], extra])
    lat_ns = rng.integers(0, 2_000_000_000, n).astype(np.uint64)  # send times around now: -1000 .. 1000 ms
    now = 1_000_000_000

    def table(keys):
        t = sbecodec.Inflight(cap, "cuda")
        m = keys.shape[0]
        st = t.remember(dev(keys.reshape(-1), torch.uint8), dev((21 * np.arange(m)).astype(np.int32), torch.int32),
                        dev(np.full(m, 21, np.int32), torch.int32), ts_default=1000)
        assert int((st != sbecodec.INF_INSERTED).sum()) == 0
        return t
    pct = sbecodec.REPORT_PERCENTILES

    def make(k):
        ts, tr = table(sent), table(recv)
        log = sbecodec.LatencyLog(log_cap, "cuda")
        log.append(sbecodec.KeyLookups(torch.full((n,), sbecodec.SENT_FIRST, dtype=torch.uint8, device="cuda"),
                                       dev(lat_ns, torch.int64), None), now, 1_000_000)
        outs = (ts.list_keys(tr, sbecodec.LIST_NOT_IN_OTHER, limit=10), tr.list_keys(ts, sbecodec.LIST_NOT_IN_OTHER, limit=10),
                log.report(pct, want_order=True))
        return ts, tr, log, outs
    R = Rot(make)
    torch.cuda.synchronize()
    # the model: std::set order is the order of the sorted byte strings
    missing = sorted(bytes(r) for r in sent[~got])
    extras = sorted(set(bytes(r) for r in extra))
    m0, e0, r0 = R.sets[0][3]
    assert int(m0.numpy()["count"][0]) == len(missing) and [r[0] for r in m0.rows()] == missing[:10]
    assert int(e0.numpy()["count"][0]) == len(extras) and [r[0] for r in e0.rows()] == extras[:10]
    d = now - lat_ns.astype(np.int64)
    lats = np.where(d >= 0, d // 1_000_000, -((-d) // 1_000_000))  # C++ division truncates toward zero
    order = np.argsort(lats, kind="stable")
    rep = r0.numpy()
    assert int(rep["count"][0]) == n and np.array_equal(rep["sorted"][:n], lats[order]) and np.array_equal(rep["order"][:n], order)
    assert list(rep["pct_index"]) == [RL.percentile_index(p, n) for p in pct]
    assert list(rep["pct_value"]) == [int(lats[order][RL.percentile_index(p, n)]) for p in pct]
    assert list(rep["stats"]) == [int(lats.sum()), int(lats.min()), int(lats.max())]

    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]

    def step(e):
        ts, tr, log, (om, oe, orp) = R.next()
        if e:
            e[0].record()
        ts.list_keys(tr, sbecodec.LIST_NOT_IN_OTHER, limit=10, out=om)
        tr.list_keys(ts, sbecodec.LIST_NOT_IN_OTHER, limit=10, out=oe)
        if e:
            e[1].record()
        log.report(pct, want_order=True, out=orp)
        if e:
            e[2].record()
    for _ in range(warmup):
        step(None)
    torch.cuda.synchronize()
    for e in ev:
        step(e)
    torch.cuda.synchronize()
    t = np.array([[e[j].elapsed_time(e[j + 1]) for j in range(2)] for e in ev])
    ms_list, ms_rep = (float(v) for v in np.median(t, axis=0))
    kernels = {"sbe_inflight_list_keys x2 (4 launches)": (ms_list, 2 * 64 * cap + 64 * (n + recv.shape[0])),
               "sbe_latency_report (memset + 25 launches)": (ms_rep, 2 * 16 * 8 * n)}
    extra_line = {"row": "delivery_report", "missing": len(missing), "extra": len(extras), "samples": n, "capacity": cap,
                  "ms_min": {"lists": float(t[:, 0].min()), "report": float(t[:, 1].min())}}
    if not NO_CPU:
        d = os.path.join(ROOT, "tests", "report")
        subprocess.run(["make", "-s", "-C", d, "report_baseline"], check=True)
        cpu = json.loads(subprocess.run([os.path.join(d, "report_baseline"), str(n)], check=True, capture_output=True,
                                        text=True).stdout)
        extra_line["cpu_set_sort_one_thread"] = cpu
        extra_line["cpu_over_device"] = cpu["report_ms"] / (ms_list + ms_rep)
    print(json.dumps(extra_line), flush=True)
    line("delivery_report", n, (ms_list + ms_rep) * 1e-3, kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="mixed,var,session,lite301,lite201,reassemble,order_json,publish_orders,materialize,autocommit,json_extract,order_select,term_scan,term_poll,term_append,commit_emit,commit_fallback,egress_step,ack_correlate,delivery_track,delivery_report")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baselines")
    ap.add_argument("--lib", help="library build to measure (A/B of variants; default: the product's)")
    ap.add_argument("--rotate", type=int, default=3, help="copies of a row's buffers the steps rotate over")
    args = ap.parse_args()
    global ROT
    ROT = args.rotate
    if args.lib:
        sbecodec.use_library(os.path.abspath(args.lib))
    global NO_CPU
    NO_CPU = args.no_cpu
    sbecodec.require_device()
    for r in args.rows.split(","):
        if r == "mixed":
            row_mixed(args.steps, args.warmup)
        elif r == "var":
            row_var(max(args.steps // 2, 5), args.warmup)
        elif r == "session":
            row_session(args.steps, args.warmup)
        elif r == "reassemble":
            row_reassemble(args.steps, args.warmup)
        elif r == "order_json":
            row_order_json(args.steps, args.warmup)
        elif r == "publish_orders":
            row_publish_orders(args.steps, args.warmup)
        elif r == "materialize":
            row_materialize(args.steps, args.warmup)
        elif r == "autocommit":
            row_autocommit(args.steps, args.warmup)
        elif r == "json_extract":
            row_json_extract(args.steps, args.warmup)
        elif r == "order_select":
            row_order_select(args.steps, args.warmup)
        elif r == "term_scan":
            row_term_scan(args.steps, args.warmup)
        elif r == "term_poll":
            row_term_poll(args.steps, args.warmup)
        elif r == "term_append":
            row_term_append(args.steps, args.warmup)
        elif r == "commit_emit":
            row_commit_emit(args.steps, args.warmup)
        elif r == "commit_fallback":
            row_commit_fallback(args.steps, args.warmup)
        elif r == "egress_step":
            row_egress_step(args.steps, args.warmup)
        elif r == "ack_correlate":
            row_ack_correlate(args.steps, args.warmup)
        elif r == "delivery_track":
            row_delivery_track(args.steps, args.warmup)
        elif r == "delivery_report":
            row_delivery_report(args.steps, args.warmup)
        elif r.startswith("lite"):
            row_lite(int(r[4:]), args.steps, args.warmup)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
