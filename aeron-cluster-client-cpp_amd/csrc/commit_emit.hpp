// commit_emit.hpp — included by sbe_codec.hip inside its anonymous namespace, after inflight.hpp
// (after every other kernel, so that the earlier device code keeps its place in the code object).
//
// The second half of ClusterClient::commit_message (src/cluster_client.cpp:626-633) for a batch
// that sbe_decode_batch(SBE_DEC_PARSE_MESSAGE) and sbe_classify_commits have been over: for every
// committed record the CommitOffsetLite (template 301) that send_commit_offset builds
// (:1264-1278, src/commit_manager.cpp:107-132) behind the SessionMessageHeader that
// send_combined_message prepends (:678-682) — sbe_emit_commit_offsets.  Only some records emit:
// the frames are compacted in record order, their message ids gathered out of the decoded input.
//
// Launches: the sizing launch (status, frame length, per-block bytes and counts), one scan over
// both block-sum arrays, the writing launch (one wave per 64-record tile through an LDS window, as
// publish_write).  No atomics: two calls give identical results.  The workspace holds the frame
// lengths and the block sums, never text.
//
// commit_fallback.hpp builds on this file: the record-level helpers below (ce_entry, ce_view,
// ce_seq, ce_session_header) and the two launch-level ones in namespace ce (size_tail, write_head)
// are the one copy both kernel pairs run.
#pragma once

// ---- one record (also compiled for the host: tests/commitsend/emit_host_check.cpp) ----
struct CeIn {
    const uint8_t* in;
    const uint64_t* rec_off;
    const uint8_t* st;         // dec->status
    const uint8_t* fl;         // dec->flags
    const uint32_t* view_off;  // [n][5]
    const uint32_t* view_len;
    const uint64_t* seq;       // or nullptr: 0 everywhere
    const uint8_t* cm;         // plan->cm
    const uint32_t* tidx;      // plan->topic_idx
    const uint64_t* last;      // plan->last (read under SBE_CE_LAST_ONLY only)
    const uint32_t* topic_id;  // [k]
    const uint8_t* iarena;     // the identifier table, clamped as the topic table is
    const uint32_t* ioff;      // [k + 1]
    uint32_t k;
    const uint8_t* mask;       // [n] or nullptr
    uint32_t flags;
    uint32_t session;
    int64_t term, sess;
};

// Entry j of an offset table over `arena` (the identifier table here, the topic table of the
// fallback): offsets clamped to the table size, a reversed entry is empty.
__device__ __forceinline__ uint32_t ce_entry(const uint8_t* arena, const uint32_t* off, uint32_t j, const uint8_t*& p) {
    const uint32_t o0 = off[j] < SBE_COMMIT_TABLE_BYTES ? off[j] : SBE_COMMIT_TABLE_BYTES;
    const uint32_t o1 = off[j + 1] < SBE_COMMIT_TABLE_BYTES ? off[j + 1] : SBE_COMMIT_TABLE_BYTES;
    p = arena + o0;
    return o1 > o0 ? o1 - o0 : 0u;
}
// Bytes [vo, vo + vl) of record i, kept inside the record whatever the descriptors say.
__device__ __forceinline__ uint32_t ce_view(const CeIn& a, uint64_t i, uint32_t vo, uint32_t vl, const uint8_t*& p) {
    const uint64_t b = a.rec_off[i], e = a.rec_off[i + 1];
    const uint64_t L64 = e > b ? e - b : 0;
    const uint32_t L = L64 > 0xffffffffull ? 0xffffffffu : (uint32_t)L64;
    const uint32_t o = vo <= L ? vo : L;
    p = a.in + b + o;
    return vl <= L - o ? vl : L - o;
}
__device__ __forceinline__ uint32_t ce_ident(const CeIn& a, uint32_t j, const uint8_t*& p) {
    return ce_entry(a.iarena, a.ioff, j, p);
}
// message_id of record i: view 2
__device__ __forceinline__ uint32_t ce_msg_id(const CeIn& a, uint64_t i, const uint8_t*& p) {
    return ce_view(a, i, a.view_off[5 * i + 2], a.view_len[5 * i + 2], p);
}
// decode writes seq only for flagged TopicMessages: every other record's sequence_number is 0
__device__ __forceinline__ uint64_t ce_seq(const CeIn& a, uint64_t i) {
    const bool has_seq = a.seq && a.st[i] == SBE_ST_TM && (a.fl[i] & (SBE_FL_SEQ_KEY | SBE_FL_SEQ_ESC));
    return has_seq ? a.seq[i] : 0ull;
}
__device__ __forceinline__ uint32_t ce_frame_len(const CeIn& a, uint32_t idn, uint32_t identn) {
    return (a.session ? SBE_SESSION_HDR_LEN : 0u) + SBE_LITE_OVERHEAD(2u) + idn + identn;
}
// The verdict of record i before the capacity is known; len: the frame's bytes (0: none).
__device__ __forceinline__ uint32_t ce_size_one(const CeIn& a, uint64_t i, uint32_t& len) {
    len = 0;
    if (a.cm[i] != SBE_CM_COMMIT || (a.mask && !a.mask[i])) return SBE_CE_NONE;
    const uint32_t j = a.tidx[i];
    if (j >= a.k || a.topic_id[j] == 0) return SBE_CE_HOST;
    if ((a.flags & SBE_CE_LAST_ONLY) && a.last[j] != i) return SBE_CE_NONE;
    const uint8_t* p;
    const uint32_t idn = ce_msg_id(a, i, p);
    if (idn > SBE_VAR_MAX_LEN) return SBE_CE_E109_MESSAGE_ID;
    len = ce_frame_len(a, idn, ce_ident(a, j, p));
    return SBE_CE_EMITTED;
}

template <class S>
__device__ __forceinline__ void ce_put16(S& s, uint32_t v) {
    s.put((uint8_t)v);
    s.put((uint8_t)(v >> 8));
}
template <class S>
__device__ __forceinline__ void ce_put64(S& s, uint64_t v) {
    for (int b = 0; b < 8; ++b) s.put((uint8_t)(v >> (8 * b)));
}
// What the frame of an emitting record holds beside the call's constants.
struct CeFields {
    uint32_t tid, idn, identn;
    uint64_t seq;
    const uint8_t *id, *ident;
};
__device__ __forceinline__ CeFields ce_fields(const CeIn& a, uint64_t i) {
    CeFields f;
    const uint32_t j = a.tidx[i];
    f.tid = a.topic_id[j];
    f.seq = ce_seq(a, i);
    f.idn = ce_msg_id(a, i, f.id);
    f.identn = ce_ident(a, j, f.ident);
    return f;
}
// The SessionMessageHeader (src/session_manager.cpp:936-967) in front of a frame, where the call asks for it.
template <class S>
__device__ __forceinline__ void ce_session_header(S& s, const CeIn& a) {
    if (!a.session) return;
    ce_put16(s, SBE_SESSION_BLOCK_LEN);
    ce_put16(s, SBE_SESSION_TEMPLATE_ID);
    ce_put16(s, SBE_CLUSTER_SCHEMA_ID);
    ce_put16(s, SBE_CLUSTER_SCHEMA_VERSION);
    ce_put64(s, (uint64_t)a.term);
    ce_put64(s, (uint64_t)a.sess);
    ce_put64(s, 0);
}
// The frame through sink s (put(byte)); copy(s, p, n) appends n bytes at p.
template <class S, class Copy>
__device__ __forceinline__ void ce_frame(S& s, const CeIn& a, const CeFields& f, Copy copy) {
    ce_session_header(s, a);
    ce_put16(s, SBE_LITE_BLOCK_LEN);
    ce_put16(s, SBE_COMMIT_OFFSET_LITE_TEMPLATE_ID);
    ce_put16(s, SBE_TOPIC_SCHEMA_ID);
    ce_put16(s, 1);
    ce_put16(s, f.tid);
    ce_put16(s, f.tid >> 16);
    ce_put64(s, f.seq);
    ce_put16(s, f.idn);
    copy(s, f.id, f.idn);
    ce_put16(s, f.identn);
    copy(s, f.ident, f.identn);
}

#ifndef COMMIT_EMIT_HOST_CHECK
namespace ce {

using namespace oj;

// What a call writes and the workspace it works in: shared by both kernel pairs (commit_fallback.hpp).
struct CeOut {
    uint64_t n;
    uint8_t* out;
    uint64_t cap;
    uint64_t* out_off;
    uint8_t* status;
    uint64_t* emit_idx;  // or nullptr
    uint64_t* totals;
    uint32_t* sz;        // [n] frame bytes (sizing launch)
    // Per block of kBlock records, nblk + 1 entries each (the last one 0), blk_cnt right behind
    // blk_bytes: frame bytes, and emitting records | SBE_CE_HOST records << 32 (n < 2^32).  One
    // exclusive scan runs over both arrays as one, so that entry nblk of blk_bytes and entry 0 of
    // blk_cnt hold the batch's bytes, and every scanned count carries that total on top.
    uint64_t* blk_bytes;
    uint64_t* blk_cnt;
};
struct CeArgs {
    CeIn c;
    CeOut o;
};

// The tail of a sizing launch, once the record's verdict st and frame bytes len are known: the
// block's sums.  Entry nblk of both sum arrays is zeroed here, so that the exclusive scan leaves
// the batch totals there.
__device__ __forceinline__ void size_tail(const CeOut& a, uint32_t st, uint32_t len, uint64_t* wtot) {
    const uint32_t lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
    uint64_t bytes, cnt;
    (void)block_excl_scan(len, wtot, lane, wv, bytes);
    (void)block_excl_scan((len ? 1ull : 0ull) | (st == SBE_CE_HOST ? 1ull << 32 : 0ull), wtot, lane, wv, cnt);
    if (threadIdx.x == 0) {
        a.blk_bytes[blockIdx.x] = bytes;
        a.blk_cnt[blockIdx.x] = cnt;
        if (blockIdx.x == 0) a.blk_bytes[gridDim.x] = a.blk_cnt[gridDim.x] = 0;
    }
}

// The head of a writing launch, for the lane whose record i = i0 + lane has a frame of len bytes
// (0: none): the frame's place [o, e) from the block's prefix, the block's records before the tile
// and the tile's scan; out_off, emit_idx and the totals stored; todo: the frame fits the capacity
// (SBE_CE_OVERFLOW stored where it does not).
struct Place {
    uint64_t o, e;
    bool todo;
};
__device__ __forceinline__ Place write_head(const CeOut& a, uint64_t i0, uint32_t lane, uint64_t len) {
    const uint64_t i = i0 + lane;
    const uint64_t bs = i0 / kBlock * kBlock;
    uint64_t pre = 0, prc = 0;
#pragma unroll
    for (uint32_t r = 0; r < kBlock / kWave; ++r) {
        const uint64_t k = bs + lane + kWave * r;
        const uint32_t s = k < i0 ? a.sz[k] : 0u;
        pre += s;
        prc += s ? 1u : 0u;
    }
    pre = a.blk_bytes[i0 / kBlock] + wave_sum64(pre);
    const uint64_t bytes_total = a.blk_cnt[0];  // what the scan carried into the counts
    prc = ((a.blk_cnt[i0 / kBlock] - bytes_total) & 0xffffffffull) + wave_sum64(prc);
    const uint64_t o = pre + wave_incl_scan64(len, (int)lane) - len, e = o + len;
    const uint64_t emitters = __ballot(len != 0);
    if (i < a.n) {
        a.out_off[i] = o;
        if (i + 1 == a.n) a.out_off[a.n] = e;
        if (len && a.emit_idx) a.emit_idx[prc + __popcll(emitters & ((1ull << lane) - 1))] = i;
    }
    if (blockIdx.x == 0 && lane == 0) {
        const uint64_t nblk = (a.n + kBlock - 1) / kBlock, c = a.blk_cnt[nblk] - bytes_total;
        a.totals[0] = c & 0xffffffffull;
        a.totals[1] = bytes_total;
        a.totals[2] = c >> 32;
    }
    const bool todo = len && e <= a.cap;
    if (len && !todo) a.status[i] = SBE_CE_OVERFLOW;
    return Place{o, e, todo};
}

// Sizing launch: status and frame bytes per record (size_tail).
__device__ __forceinline__ void emit_measure_block(const CeArgs& a) {
    __shared__ uint64_t wtot[kBlock / kWave];
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t len = 0, st = SBE_CE_NONE;
    if (i < a.o.n) {
        st = ce_size_one(a.c, i, len);
        a.o.status[i] = (uint8_t)st;
        a.o.sz[i] = len;
    }
    size_tail(a.o, st, len, wtot);
}
__global__ __launch_bounds__(kBlock) void commit_emit_measure(CeArgs a) { emit_measure_block(a); }

// The *_counted launches: o.n is the capacity the grids, the workspace and the block-sum arrays were
// laid out by.  A sizing block past the count leaves zero sums (size_tail on records without
// frames), so one scan over the arrays of the capacity gives the prefixes and totals of the count.
// A writing tile past the count exits, but for tile 0, which stores the totals (and out_off[0] of
// an empty batch).
__device__ __forceinline__ bool counted_write_tile(CeOut& o, const uint64_t* n_dev) {
    o.n = counted_n(n_dev, o.n);
    if (o.n == 0 && blockIdx.x == 0 && threadIdx.x == 0) o.out_off[0] = 0;
    return blockIdx.x == 0 || (uint64_t)blockIdx.x * kWWave < o.n;
}
__global__ __launch_bounds__(kBlock) void commit_emit_measure_counted(CeArgs a, const uint64_t* n_dev) {
    a.o.n = counted_n(n_dev, a.o.n);
    emit_measure_block(a);
}
// Writing launch: one wave per tile of 64 records.  A typical framed record is ~100 bytes (32 + 24
// + a 36-byte id + a short identifier), so a tile's frames fit the window in one pass; a frame
// larger than the window goes from its lane straight to HBM (write_staged).  Every frame is at
// least 24 bytes, which write_staged's window passes rely on.
#ifndef SBE_CE_WIN
#define SBE_CE_WIN 8192
#endif
constexpr uint32_t kCeWin = SBE_CE_WIN;
static_assert(kCeWin >= 4096 && kCeWin % 16 == 0 && kBlock % kWWave == 0, "a writing tile lies inside one sizing block");

__device__ __forceinline__ void emit_write_tile(const CeArgs& a) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kCeWin];
    const uint32_t lane = threadIdx.x;
    const uint64_t i0 = (uint64_t)blockIdx.x * kWWave, i = i0 + lane;
    // this record's length and, for an emitter, everything its frame holds: loaded first, so that
    // the loads are in flight while the offsets are worked out
    const uint64_t len = i < a.o.n ? a.o.sz[i] : 0;
    CeFields f{};
    if (len) f = ce_fields(a.c, i);
    const auto [o, e, todo] = write_head(a.o, i0, lane, len);
    write_staged<kCeWin>(a.o.out, (lw8*)win, lane, todo, o, e, [&](auto& s) {
        ce_frame(s, a.c, f, [](auto& t, const uint8_t* p, uint32_t m) { t = pub::raw(t, (gu8*)p, m); });
    });
}
__global__ __launch_bounds__(kWWave) void commit_emit_write(CeArgs a) { emit_write_tile(a); }
__global__ __launch_bounds__(kWWave) void commit_emit_write_counted(CeArgs a, const uint64_t* n_dev) {
    if (counted_write_tile(a.o, n_dev)) emit_write_tile(a);
}

}  // namespace ce
#endif
