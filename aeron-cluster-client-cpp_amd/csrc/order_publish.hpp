// order_publish.hpp — ClusterClient::publish_order for a batch of Orders, fused on the GPU
// (included by sbe_codec.hip after every other kernel, so that the earlier device code keeps its
// place in the code object; it needs order_json.hpp).
//
// Replaces, per Order, the whole of publish_order (src/cluster_client.cpp:300-333, :335-372):
// Order::validate (src/order_types.cpp:66-120), the messageType choice (:309-312), Order::to_json,
// the headers JSON, create_topic_message (src/session_manager.cpp:1050-1115) and the
// SessionMessageHeader send_combined_message prepends (:1118-1144).  The two JSON texts are never
// written to HBM on their own: the sizing launch counts them (CountSink), the writing launch
// composes each record — framing, header, block, the five length-prefixed fields — through the
// same sinks order_json.hpp writes its texts with, into the wave's LDS window, and stores the
// window with coalesced 16-byte stores.
//
// Launches: per-block string totals and their scans (packed arenas only), the sizing launch
// (validation, text lengths, E109, record lengths, per-block record bytes), one scan of the block
// sums, the writing launch.
#pragma once

namespace pub {

using namespace oj;

struct PubArgs {
    JsonArgs j;  // the Order batch, out / cap / out_off / status, sz (record bytes), str_base, blk_str, blk_txt
    // the members only validate() reads (chk_len == nullptr: no validation)
    const uint8_t* chk_arena;
    const uint32_t* chk_off;  // [n][2] or nullptr = packed
    const uint32_t* chk_len;  // [n][2] order_type, time_in_force
    const double* limit_price;
    const double* stop_price;
    const uint8_t* present;   // bit 0 stop_price, bit 1 expiry_timestamp
    uint64_t* blk_chk;        // per block: packed checks-arena bytes, then their exclusive scan
    const uint8_t* topic;
    uint32_t topic_len;
    const uint64_t* tm_ts;    // TopicMessage timestamp [n] or nullptr; 0 -> ts_default
    uint64_t ts_default;
    uint32_t cut;             // 8 under SBE_ENC_REF_TRUNCATE8, else 0
    uint32_t session;         // 1: the 32-byte SessionMessageHeader first
    int64_t term, sess;
    uint16_t* mask;           // [n] or nullptr
    uint32_t* tl;             // [n][2] payload / headers text lengths (sizing launch)
};

// ---- validation (src/order_types.cpp:66-120, :455-467) ----
template <class P, size_t N>
__device__ inline bool str_is(P p, uint32_t n, const char (&t)[N]) {  // exact match
    if (n != N - 1) return false;
    BlockReader<P> rd;
    bool eq = true;
#pragma unroll
    for (size_t k = 0; k + 1 < N; ++k) eq = eq && rd.at(p + k) == (uint32_t)(uint8_t)t[k];
    return eq;
}

// All of validate()'s messages as a bit mask, bit k = message k in the reference's order
// (SBE_PUB_INVALID_ID + k).  The comparisons are the reference's: `x <= 0.0` is false for NaN.
template <class P>
__device__ inline uint32_t validate(const PubArgs& a, uint64_t i, P side, const uint32_t l[kFields], gu8* ot,
                                    uint32_t otl, gu8* tif, uint32_t tifl) {
    uint32_t m = 0;
    if (l[5] == 0) m |= 1u << 0;
    if (l[2] == 0) m |= 1u << 1;
    if (l[3] == 0) m |= 1u << 2;
    if (!(str_is(side, l[4], "BUY") || str_is(side, l[4], "SELL"))) m |= 1u << 3;
    if (a.j.quantity[i] <= 0.0) m |= 1u << 4;
    const bool limit = str_is(ot, otl, "LIMIT"), stop = str_is(ot, otl, "STOP"),
               stop_limit = str_is(ot, otl, "STOP_LIMIT");
    if (!(limit || stop || stop_limit || str_is(ot, otl, "MARKET"))) m |= 1u << 5;
    const bool lim_bad = a.limit_price[i] <= 0.0;
    const bool stop_bad = !(a.present[i] & 1u) || a.stop_price[i] <= 0.0;
    if (limit && lim_bad) m |= 1u << 6;
    if (stop && stop_bad) m |= 1u << 7;
    if (stop_limit && stop_bad) m |= 1u << 8;
    if (stop_limit && lim_bad) m |= 1u << 9;
    const bool gtd = str_is(tif, tifl, "GTD");
    if (!(gtd || str_is(tif, tifl, "GTC") || str_is(tif, tifl, "IOC") || str_is(tif, tifl, "FOK") ||
          str_is(tif, tifl, "DAY")))
        m |= 1u << 10;
    if (gtd && !(a.present[i] & 2u)) m |= 1u << 11;
    return m;
}

// Packed arenas: each block's Order string bytes into blk_str, checks string bytes into blk_chk.
__global__ __launch_bounds__(kBlock) void publish_totals(PubArgs a) {
    __shared__ uint64_t wtot[kBlock / kWave];
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
    const bool chk = a.chk_len && !a.chk_off;
    uint64_t t = 0, c = 0, total;
    if (i < a.j.n) {
        if (!a.j.str_off)
            for (uint32_t k = 0; k < kFields; ++k) t += a.j.str_len[kFields * i + k];
        if (chk) c = (uint64_t)a.chk_len[2 * i] + a.chk_len[2 * i + 1];
    }
    if (!a.j.str_off) {  // uniform over the launch
        (void)block_excl_scan(t, wtot, lane, wv, total);
        if (threadIdx.x == 0) a.j.blk_str[blockIdx.x] = total;
    }
    if (chk) {
        (void)block_excl_scan(c, wtot, lane, wv, total);
        if (threadIdx.x == 0) a.blk_chk[blockIdx.x] = total;
    }
}

// One Order's verdict and sizes: validation first (a validation status wins over E109), then
// computeLength's order topic, messageType, uuid, payload, headers on the text lengths.
template <class P>
__device__ __forceinline__ uint64_t size_one(const PubArgs& a, uint64_t i, P const f[kFields], const uint32_t l[kFields],
                                         uint64_t chk_at) {
    CountSink p;
    order_text<SBE_JSON_ORDER_PAYLOAD>(p, a.j, i, f, l);
    CountSink h;
    order_text<SBE_JSON_PUBLISH_HEADERS>(h, a.j, i, f, l);
    uint32_t m = 0;
    if (a.chk_len) {
        const uint32_t otl = a.chk_len[2 * i], tifl = a.chk_len[2 * i + 1];
        const uint64_t o0 = a.chk_off ? a.chk_off[2 * i] : chk_at;
        const uint64_t o1 = a.chk_off ? a.chk_off[2 * i + 1] : chk_at + otl;
        m = validate(a, i, f[4], l, (gu8*)(a.chk_arena + o0), otl, (gu8*)(a.chk_arena + o1), tifl);
    }
    uint32_t st = SBE_ENC_OK;
    if (m) st = SBE_PUB_INVALID_ID + (uint32_t)__builtin_ctz(m);
    else if (a.topic_len > SBE_VAR_MAX_LEN) st = SBE_ENC_E109_TOPIC;
    else if (l[6] > SBE_VAR_MAX_LEN) st = SBE_ENC_E109_UUID;
    else if (p.n > SBE_VAR_MAX_LEN) st = SBE_ENC_E109_PAYLOAD;
    else if (h.n > SBE_VAR_MAX_LEN) st = SBE_ENC_E109_HEADERS;
    const uint64_t len = (a.session ? SBE_SESSION_HDR_LEN : 0u) + SBE_TM_WIRE_OVERHEAD - a.cut + a.topic_len + 12u +
                         l[6] + p.n + h.n;
    a.j.sz[i] = st == SBE_ENC_OK ? len : 0;
    a.tl[2 * i] = (uint32_t)(p.n < 0xffffffffull ? p.n : 0xffffffffull);
    a.tl[2 * i + 1] = (uint32_t)(h.n < 0xffffffffull ? h.n : 0xffffffffull);
    if (a.j.status) a.j.status[i] = (uint8_t)st;
    if (a.mask) a.mask[i] = (uint16_t)m;
    return st == SBE_ENC_OK ? len : 0;
}

// Sizing launch.  The packed-arena staging is order_json_measure's (stage_wave_strings): a range
// larger than the wave's LDS share, and the str_off form, are read from HBM.
__global__ __launch_bounds__(kBlock) void publish_measure(PubArgs a) {
    __shared__ uint64_t wtot[kBlock / kWave];
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < a.j.n;
    const uint32_t lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
    uint32_t l[kFields];
    uint64_t tot = 0, total;
    if (live)
        for (uint32_t k = 0; k < kFields; ++k) {
            l[k] = a.j.str_len[kFields * i + k];
            tot += l[k];
        }
    uint64_t chk_at = 0;
    if (a.chk_len && !a.chk_off) {  // uniform over the launch
        const uint64_t c = live ? (uint64_t)a.chk_len[2 * i] + a.chk_len[2 * i + 1] : 0;
        chk_at = a.blk_chk[blockIdx.x] + block_excl_scan(c, wtot, lane, wv, total);
    }
    bool done = false;
    uint64_t base = 0, rec = 0;  // rec: this Order's record bytes (0: nothing emitted)
    if (!a.j.str_off) {  // uniform over the launch
        base = a.j.blk_str[blockIdx.x] + block_excl_scan(tot, wtot, lane, wv, total);
        if (live) a.j.str_base[i] = base;
        __shared__ __attribute__((aligned(16))) uint8_t sbuf[kBlock / kWave][SBE_OJ_MSTR];
        uint64_t g0 = 0;
        const bool staged = stage_wave_strings<SBE_OJ_MSTR>(a.j.arena, sbuf[wv], base, tot, a.j.n, i - lane, lane, g0);
        __syncthreads();
        if (staged && live) {
            lr8* f[kFields];
            uint64_t at = base - g0;
            for (uint32_t k = 0; k < kFields; ++k) {
                f[k] = (lr8*)(sbuf[wv] + at);
                at += l[k];
            }
            rec = size_one(a, i, f, l, chk_at);
        }
        done = staged;
    }
    if (!done && live) {
        gu8* f[kFields];
        uint64_t at = base;
        for (uint32_t k = 0; k < kFields; ++k) {
            f[k] = (gu8*)(a.j.arena + (a.j.str_off ? (uint64_t)a.j.str_off[kFields * i + k] : at));
            at += l[k];
        }
        rec = size_one(a, i, f, l, chk_at);
    }
    (void)block_excl_scan(rec, wtot, lane, wv, total);
    if (threadIdx.x == 0) a.j.blk_txt[blockIdx.x] = total;
}

// ---- the record ----
// A sink that drops what lies past the record's emitted length: under SBE_ENC_REF_TRUNCATE8 the
// last 8 bytes of the record (always headers text: its skeleton alone is 58 bytes) are not emitted.
template <class S>
struct CutSink {
    S s;
    uint64_t left;
    __device__ CutSink(const S& q, uint64_t room) : s(q), left(room) {}
    __device__ void put(uint8_t b) {
        if (left) s.put(b), --left;
    }
    __device__ void run(const uint4& v, uint32_t o, uint32_t m) {
        const uint32_t k = m < left ? m : (uint32_t)left;
        if (k) s.run(v, o, k);
        left -= k;
    }
};

template <class S>
__device__ inline void put16(S& s, uint32_t v) {
    s.put((uint8_t)v);
    s.put((uint8_t)(v >> 8));
}
template <class S>
__device__ inline void put64(S& s, uint64_t v) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s.put((uint8_t)(v >> (8 * k)));
}

// len bytes at p unchanged (topic, uuid), a 16-byte block at a time
template <class S>
__device__ OJ_HELPER S raw(S s, gu8* p, uint64_t len) {
    BlockReader<gu8*> rd;
    for (uint64_t i = 0; i < len;) {
        (void)rd.at(p + i);
        const uint32_t o = (uint32_t)((uintptr_t)(p + i) & 15);
        const uint64_t left = len - i;
        const uint32_t m = left < 16 - o ? (uint32_t)left : 16 - o;
        s.run(rd.v, o, m);
        i += m;
    }
    return s;
}

// Record i: `emit` bytes in all (the sizing launch's sz[i]).
template <class S>
__device__ __forceinline__ void record(S& s, const PubArgs& a, uint64_t i, gu8* const f[kFields],
                                       const uint32_t l[kFields], uint32_t plen, uint32_t hlen, uint64_t emit) {
    if (a.session) {  // SessionMessageHeader (src/session_manager.cpp:936-967)
        put16(s, SBE_SESSION_BLOCK_LEN);
        put16(s, SBE_SESSION_TEMPLATE_ID);
        put16(s, SBE_CLUSTER_SCHEMA_ID);
        put16(s, SBE_CLUSTER_SCHEMA_VERSION);
        put64(s, (uint64_t)a.term);
        put64(s, (uint64_t)a.sess);
        put64(s, 0);
    }
    put16(s, SBE_TM_BLOCK_LEN);
    put16(s, SBE_TM_TEMPLATE_ID);
    put16(s, SBE_TOPIC_SCHEMA_ID);
    put16(s, 1);
    const uint64_t ts = a.tm_ts ? a.tm_ts[i] : 0;
    put64(s, ts ? ts : a.ts_default);
    put64(s, 0);  // sequenceNumber
    put16(s, a.topic_len);
    s = raw(s, (gu8*)a.topic, a.topic_len);
    put16(s, 12);
    if (is_update_status(f[7], l[7])) lit(s, "UPDATE_ORDER");
    else lit(s, "CREATE_ORDER");
    put16(s, l[6]);
    s = raw(s, f[6], l[6]);
    put16(s, plen);
    order_text<SBE_JSON_ORDER_PAYLOAD>(s, a.j, i, f, l);
    put16(s, hlen);
    CutSink<S> c(s, emit - s.n);
    order_text<SBE_JSON_PUBLISH_HEADERS>(c, a.j, i, f, l);
    s = c.s;
}

// Writing launch: one wave per kPubOpw Orders, as order_json_write.  A typical framed record is
// ~760 bytes (32 + 26 + topic + 12 + 29 + ~560 + ~95), so 32 of them fit the window in one pass.
#ifndef SBE_PUB_WIN
#define SBE_PUB_WIN 26624
#endif
#ifndef SBE_PUB_OPW
#define SBE_PUB_OPW 32
#endif
#ifndef SBE_PUB_MINW  // waves per SIMD the writing launch's registers must allow (2: at most 256)
#define SBE_PUB_MINW 2
#endif
constexpr uint32_t kPubWin = SBE_PUB_WIN, kPubOpw = SBE_PUB_OPW;
static_assert(kPubWin >= 4096 && kPubWin % 16 == 0, "the window must hold a typical record");
static_assert(kBlock % kPubOpw == 0 && kPubOpw <= kWWave, "a writing tile lies inside one sizing block");

__global__ __launch_bounds__(kWWave, SBE_PUB_MINW) void publish_write(PubArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kPubWin];
    const uint32_t lane = threadIdx.x;
    const uint64_t i0 = (uint64_t)blockIdx.x * kPubOpw, i = i0 + lane;
    const bool live = lane < kPubOpw && i < a.j.n;
    // record offsets: the block's prefix, the sizes of the block's Orders before the tile, the tile's scan
    const uint64_t bs = i0 / kBlock * kBlock;
    uint64_t pre = 0;
#pragma unroll
    for (uint32_t r = 0; r < kBlock / kWave; ++r) {
        const uint64_t k = bs + lane + kWave * r;
        if (k < i0) pre += a.j.sz[k];
    }
    pre = a.j.blk_txt[i0 / kBlock] + wave_sum64(pre);
    const uint64_t len = live ? a.j.sz[i] : 0;
    const uint64_t o = pre + wave_incl_scan64(len, (int)lane) - len, e = o + len;
    if (live) {
        a.j.out_off[i] = o;
        if (i + 1 == a.j.n) a.j.out_off[a.j.n] = e;
    }
    const bool todo = live && len && e <= a.j.cap;
    if (live && len && !todo && a.j.status) a.j.status[i] = SBE_ENC_OVERFLOW;
    uint32_t l[kFields];
    gu8* f[kFields];
    uint32_t plen = 0, hlen = 0;
    if (todo) {
        plen = a.tl[2 * i];
        hlen = a.tl[2 * i + 1];
        uint64_t at = a.j.str_off ? 0 : a.j.str_base[i];
        for (uint32_t k = 0; k < kFields; ++k) {
            l[k] = a.j.str_len[kFields * i + k];
            f[k] = (gu8*)(a.j.arena + (a.j.str_off ? (uint64_t)a.j.str_off[kFields * i + k] : at));
            at += l[k];
        }
    }
    write_staged<kPubWin>(a.j.out, (lw8*)win, lane, todo, o, e,
                          [&](auto& s) { record(s, a, i, f, l, plen, hlen, len); });
}

}  // namespace pub
