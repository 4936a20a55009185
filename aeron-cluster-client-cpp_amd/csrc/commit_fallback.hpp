// commit_fallback.hpp — included by sbe_codec.hip inside its anonymous namespace, after
// commit_emit.hpp (after every other kernel, so that the earlier device code keeps its place in
// the code object).
//
// sbe_emit_commit_offsets_ex with a fallback: the records sbe_emit_commit_offsets leaves to the
// host as SBE_CE_HOST because their topic has no numeric id get the frame the reference sends for
// them, CommitManager::build_commit_offset_message's legacy branch (src/commit_manager.cpp:134-175):
// a TopicMessage on "_subscriptions" of type "COMMIT_OFFSET" whose payload is the jsoncpp text of
// the CommitOffset (indentation "", keys sorted) and whose uuid is "commit_offset_" + identifier +
// "_" + a clock reading, behind the SessionMessageHeader.  A record whose topic token is not in
// the table but is one of topic_to_id's four names (:16-22) gets its CommitOffsetLite.
//
// The reference's two length quirks are kept: putUuid / putPayload take the length as
// std::uint16_t (TopicMessage.h:865-879 and the payload twin), so each field holds len mod 65536
// and that many leading bytes; and the flyweight is wrapped over a 1048-byte buffer with
// wrapForEncode(buf, 8, 1040), positions absolute, so a record of more than 1040 bytes throws
// "buffer too short [E100]" (SBE_CE_E100_FALLBACK, 0 bytes).
//
// Launches as commit_emit.hpp: sizing (the text is measured with a counting sink), the scan over
// the block sums, writing (the record composed straight into the LDS window; the payload clipped
// by a sink that stops).  The workspace holds lengths and block sums, never text.  The block sums
// of the sizing launch and the offsets, ranks and totals of the writing launch are commit_emit.hpp's
// (ce::size_tail, ce::write_head), as are the clamped table entry, the view kept inside its
// record, the sequence rule and the session header (ce_entry, ce_view, ce_seq, ce_session_header).
#pragma once

// ---- one record (also compiled for the host: tests/commitfallback/fallback_host_check.cpp) ----
struct CfIn {
    CeIn c;
    const uint64_t* ts;        // dec->ts
    const uint8_t* kind;       // plan->topic_kind
    const uint32_t* tok_off;   // plan->topic_off
    const uint32_t* tok_len;   // plan->topic_len
    const uint8_t* tarena;     // the classify call's topic table, clamped as there
    const uint32_t* toff;      // [k + 1]
    const uint8_t* dident;     // the identifier of records outside the table
    uint32_t didentn;
    uint64_t now_ns, uuid_ns;
};

constexpr uint32_t kCfRecMax = 1040;   // m_bufferLength of wrapForEncode(buf, 8, 1048 - 8)
constexpr uint32_t kCfRecFixed = 63;   // header 8, block 16, 2+14, 2+13, 2 (uuid), 2 (payload), 2+2

// A sink of the fallback frame: put(b) appends while `left` allows.  The frame starts with left =
// its sized length, so a lane never writes outside its own bytes; a field is clipped by lowering
// left for its duration.
template <class S, class F>
__device__ __forceinline__ void cf_clipped(S& s, uint64_t m, F body) {
    const uint64_t room = s.left, lim = m < room ? m : room;
    s.left = lim;
    body();
    s.left = room - (lim - s.left);
}
template <class S, size_t N>
__device__ __forceinline__ void cf_lit(S& s, const char (&t)[N]) {
#pragma unroll
    for (size_t k = 0; k + 1 < N; ++k) s.put((uint8_t)t[k]);
}
__device__ __forceinline__ uint32_t cf_ndig(uint64_t v) {  // decimal digits of v (1 for 0)
    uint32_t d = 1;
    for (uint64_t p = 10; d < 20 && v >= p; p *= 10) ++d;
    return d;
}

// topic_to_id (src/commit_manager.cpp:16-22) on a byte range
__device__ __forceinline__ uint32_t cf_name_id(const uint8_t* p, uint32_t n) {
    const char* nm;
    uint32_t id;
    switch (n) {
        case 19: nm = "order_request_topic"; id = 1; break;
        case 24: nm = "order_notification_topic"; id = 2; break;
        case 6: nm = "orders"; id = 3; break;
        case 26: nm = "order_status_request_topic"; id = 4; break;
        default: return 0;
    }
    for (uint32_t k = 0; k < n; ++k)
        if (p[k] != (uint8_t)nm[k]) return 0;
    return id;
}

// What a record that sbe_emit_commit_offsets reports as SBE_CE_HOST becomes under a fallback.
enum : uint32_t { kCfHost = 0, kCfSkip = 1, kCfLite = 2, kCfJson = 3 };
struct CfRec {
    uint32_t what;  // kCf*
    uint32_t tid;   // kCfLite: topic_to_id of the token
    uint32_t idn, identn, topicn;
    uint64_t seq, ts, uuid;
    const uint8_t *id, *ident, *topic;
};
__device__ __forceinline__ CfRec cf_record(const CfIn& a, uint64_t i) {
    CfRec r{};
    const uint32_t j = a.c.tidx[i];
    if (j < a.c.k) {  // an entry without an id (ce_size_one has taken the others)
        if ((a.c.flags & SBE_CE_LAST_ONLY) && a.c.last[j] != i) {
            r.what = kCfSkip;
            return r;
        }
        r.what = kCfJson;
        r.topicn = ce_entry(a.tarena, a.toff, j, r.topic);  // clamped as the classifier clamps it
        r.identn = ce_ident(a.c, j, r.ident);
    } else if (j == SBE_TOPIC_UNKNOWN && a.kind[i] == SBE_TOPIC_KIND_STRING) {
        r.topicn = ce_view(a.c, i, a.tok_off[i], a.tok_len[i], r.topic);  // the topic token
        r.ident = a.dident;
        r.identn = a.didentn;
        r.tid = cf_name_id(r.topic, r.topicn);
        r.what = r.tid ? kCfLite : kCfJson;
    } else {
        r.what = kCfHost;
        return r;
    }
    r.seq = ce_seq(a.c, i);
    r.ts = a.ts[i];
    r.uuid = a.uuid_ns + i;
    r.idn = ce_msg_id(a.c, i, r.id);
    return r;
}
// The fields of a kCfLite record's frame: a CommitOffsetLite through ce_frame.
__device__ __forceinline__ CeFields cf_lite_fields(const CfRec& r) {
    return CeFields{r.tid, r.idn, r.identn, r.seq, r.id, r.ident};
}

// The text (commit_manager.cpp:135-145, = serialize_commit_offset :197-209) through sink s.
// quote(s, p, n) appends valueToQuotedStringN(p, n, emitUTF8 = false), dec(s, v) the decimal.
// A string is handed over only as far as the sink can still take it: every input byte yields at
// least one output byte, and 4 bytes more keep a UTF-8 sequence that straddles the cut whole.
template <class S, class Quote, class Dec>
__device__ __forceinline__ void cf_text(S& s, const CfRec& r, Quote quote, Dec dec) {
    auto q = [&](const uint8_t* p, uint32_t n) {
        if (!s.left) return;
        const uint64_t take = s.left > 0xfffffff0ull ? 0xffffffffull : s.left + 4;
        quote(s, p, n < take ? n : (uint32_t)take);
    };
    cf_lit(s, "{\"action\":\"COMMIT_OFFSET\",\"messageIdentifier\":");
    q(r.ident, r.identn);
    cf_lit(s, ",\"message_id\":");
    q(r.id, r.idn);
    cf_lit(s, ",\"sequence_number\":");
    dec(s, r.seq);
    cf_lit(s, ",\"timestamp_nanos\":");
    dec(s, r.ts);
    cf_lit(s, ",\"topic\":");
    q(r.topic, r.topicn);
    s.put('}');
}

// uuid and payload lengths as the u16 overloads store them; rec: the record's bytes
__device__ __forceinline__ uint32_t cf_uuid_len(const CfRec& r) {
    return (14u + r.identn + 1u + cf_ndig(r.uuid)) & 0xffffu;
}
// The verdict for a kCfJson record whose text is text_len bytes long.
__device__ __forceinline__ uint32_t cf_json_len(const CfIn& a, const CfRec& r, uint64_t text_len, uint32_t& len) {
    const uint32_t rec = kCfRecFixed + cf_uuid_len(r) + (uint32_t)(text_len & 0xffffu);
    len = rec > kCfRecMax ? 0u : (a.c.session ? SBE_SESSION_HDR_LEN : 0u) + rec;
    return len ? SBE_CE_EMITTED_JSON : SBE_CE_E100_FALLBACK;
}
// The verdict of record i before the capacity is known; text_len(r): the bytes of r's text.
template <class TextLen>
__device__ __forceinline__ uint32_t cf_size_one(const CfIn& a, uint64_t i, uint32_t& len, TextLen text_len) {
    const uint32_t st = ce_size_one(a.c, i, len);
    if (st != SBE_CE_HOST) return st;
    const CfRec r = cf_record(a, i);
    if (r.what == kCfHost) return SBE_CE_HOST;
    if (r.what == kCfSkip) return SBE_CE_NONE;
    if (r.what == kCfLite) {
        if (r.idn > SBE_VAR_MAX_LEN) return SBE_CE_E109_MESSAGE_ID;
        len = ce_frame_len(a.c, r.idn, r.identn);
        return SBE_CE_EMITTED;
    }
    return cf_json_len(a, r, text_len(r), len);
}

// The JSON frame of `len` bytes through sink s (s.left >= len); copy(s, p, n) appends n bytes.
template <class S, class Copy, class Quote, class Dec>
__device__ __forceinline__ void cf_frame(S& s, const CfIn& a, const CfRec& r, uint32_t len, Copy copy, Quote quote,
                                         Dec dec) {
    const uint32_t u = cf_uuid_len(r);
    const uint32_t p = len - (a.c.session ? SBE_SESSION_HDR_LEN : 0u) - kCfRecFixed - u;
    ce_session_header(s, a.c);
    ce_put16(s, SBE_TM_BLOCK_LEN);
    ce_put16(s, SBE_TM_TEMPLATE_ID);
    ce_put16(s, SBE_TOPIC_SCHEMA_ID);
    ce_put16(s, 1);
    ce_put64(s, a.now_ns);
    ce_put64(s, 0);  // sequenceNumber
    ce_put16(s, 14);
    cf_lit(s, "_subscriptions");
    ce_put16(s, 13);
    cf_lit(s, "COMMIT_OFFSET");
    ce_put16(s, u);
    cf_clipped(s, u, [&] {
        cf_lit(s, "commit_offset_");
        copy(s, r.ident, r.identn);
        s.put('_');
        dec(s, r.uuid);
    });
    ce_put16(s, p);
    cf_clipped(s, p, [&] { cf_text(s, r, quote, dec); });
    ce_put16(s, 2);
    cf_lit(s, "{}");
}

#ifndef COMMIT_EMIT_HOST_CHECK
namespace cf {

using namespace oj;

// The sinks of these kernels are types of their own, so that the out-of-line string helpers
// (oj::quoted, pub::raw) are instantiated for these kernels alone and the instances the earlier
// kernels call keep their register allocation.
struct CountOut {
    uint64_t n = 0, left = ~0ull;
    __device__ void put(uint8_t) {
        if (left) ++n, --left;
    }
    __device__ void run(const uint4&, uint32_t, uint32_t m) {
        const uint64_t k = m < left ? m : left;
        n += k;
        left -= k;
    }
};
template <class S>
struct ClipOut {
    S s;
    uint64_t left;
    __device__ ClipOut(const S& q, uint64_t room) : s(q), left(room) {}
    __device__ void put(uint8_t b) {
        if (left) s.put(b), --left;
    }
    __device__ void run(const uint4& v, uint32_t o, uint32_t m) {
        const uint32_t k = m < left ? m : (uint32_t)left;
        if (k) s.run(v, o, k);
        left -= k;
    }
};

struct CfArgs {
    CfIn f;
    ce::CeOut o;
};

__device__ __forceinline__ uint64_t text_bytes(const CfRec& r) {
    CountOut c;
    cf_text(c, r, [](CountOut& t, const uint8_t* p, uint32_t m) { t = quoted(t, (gu8*)p, (uint64_t)m); },
            [](CountOut& t, uint64_t v) { dec_u64(t, v); });
    return c.n;
}

// Sizing launch: as commit_emit_measure, the text of a JSON record measured on the way.
__device__ __forceinline__ void fallback_measure_block(const CfArgs& a) {
    __shared__ uint64_t wtot[kBlock / kWave];
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t len = 0, st = SBE_CE_NONE;
    if (i < a.o.n) {
        st = cf_size_one(a.f, i, len, [](const CfRec& r) { return text_bytes(r); });
        a.o.status[i] = (uint8_t)st;
        a.o.sz[i] = len;
    }
    ce::size_tail(a.o, st, len, wtot);
}
__global__ __launch_bounds__(kBlock) void commit_fallback_measure(CfArgs a) { fallback_measure_block(a); }
// the *_counted launches: as commit_emit_measure_counted / commit_emit_write_counted
__global__ __launch_bounds__(kBlock) void commit_fallback_measure_counted(CfArgs a, const uint64_t* n_dev) {
    a.o.n = counted_n(n_dev, a.o.n);
    fallback_measure_block(a);
}

// Writing launch: one wave per tile of 64 records, as commit_emit_write.  A JSON frame with short
// strings is ~290 bytes (32 + 63 + a ~45-byte uuid + a ~150-byte text) and at most 1072, so a tile
// of them is 18 to 67 KiB: the window is refilled several times a tile (write_staged's passes),
// and each pass composes only the lanes whose frames it holds.  The lanes at work per CU are then
// bounded by the LDS a CU has, whatever the window: a larger one takes fewer passes per wave and
// fits fewer waves.  16 KiB holds a tile of short-string frames in one or two passes.
#ifndef SBE_CF_WIN
#define SBE_CF_WIN 16384
#endif
constexpr uint32_t kCfWin = SBE_CF_WIN;
static_assert(kCfWin >= 4096 && kCfWin % 16 == 0 && kCfWin <= 65536, "the window holds several whole frames");
#ifndef SBE_CF_MINW  // waves per SIMD the writing launch's registers must allow (2: at most 256)
#define SBE_CF_MINW 2
#endif

__device__ __forceinline__ void fallback_write_tile(const CfArgs& a) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kCfWin];
    const uint32_t lane = threadIdx.x;
    const uint64_t i0 = (uint64_t)blockIdx.x * kWWave, i = i0 + lane;
    const uint64_t len = i < a.o.n ? a.o.sz[i] : 0;
    // an emitter's fields: a table entry with an id as commit_emit_write has them, the others from
    // cf_record (a Lite frame of a named token through the same CeFields)
    bool json = false;
    CeFields f{};
    CfRec r{};
    if (len) {
        const uint32_t j = a.f.c.tidx[i];
        if (j < a.f.c.k && a.f.c.topic_id[j] != 0) {
            f = ce_fields(a.f.c, i);
        } else {
            r = cf_record(a.f, i);
            json = r.what == kCfJson;
            f = cf_lite_fields(r);
        }
    }
    const auto [o, e, todo] = ce::write_head(a.o, i0, lane, len);
    write_staged<kCfWin>(a.o.out, (lw8*)win, lane, todo, o, e, [&](auto& s0) {
        typedef ClipOut<std::remove_reference_t<decltype(s0)>> Out;
        Out s(s0, len);
        auto copy = [](Out& t, const uint8_t* p, uint32_t m) { t = pub::raw(t, (gu8*)p, (uint64_t)m); };
        if (json)
            cf_frame(s, a.f, r, (uint32_t)len, copy,
                     [](Out& t, const uint8_t* p, uint32_t m) { t = quoted(t, (gu8*)p, (uint64_t)m); },
                     [](Out& t, uint64_t v) { dec_u64(t, v); });
        else
            ce_frame(s, a.f.c, f, copy);
    });
}
__global__ __launch_bounds__(kWWave, SBE_CF_MINW) void commit_fallback_write(CfArgs a) { fallback_write_tile(a); }
__global__ __launch_bounds__(kWWave, SBE_CF_MINW) void commit_fallback_write_counted(CfArgs a, const uint64_t* n_dev) {
    if (ce::counted_write_tile(a.o, n_dev)) fallback_write_tile(a);
}

}  // namespace cf
#endif
