// order_select.hpp — included by sbe_codec.hip inside its anonymous namespace, after delivery_report.hpp.
//
// The first line of the subscriber's callback (examples/pubsub_reconnect_test.cpp:578-579) for a
// decoded batch: the ParseResult predicates of include/aeron_cluster/sbe_messages.hpp:332-406 and
// classify_topic of include/aeron_cluster/topic_router.hpp, per record, on the device
// (sbe_order_select).  The input is what sbe_decode_batch(SBE_DEC_PARSE_MESSAGE) wrote for the same
// in / rec_off; which strings and header fields a record's ParseResult has follows the host mirror's
// materialize_into:
//   SBE_ST_TM             type view 1, payload view 3, hdr
//   SBE_ST_ACK            type "Acknowledgment", payload view 1 ("SUCCESS" under SBE_FL_PAYLOAD_DEFAULT), hdr
//   SBE_ST_SESSION_EVENT  type "SessionEvent", payload view 3, hdr
//   error statuses        no strings, hdr all zero (SBE_ST_ERR_UNKNOWN_TYPE keeps hdr)
//   anything else         pred = 0 (no ParseResult exists)
// The fixed types and "SUCCESS" contain none of the searched words.  Every view is kept inside its
// record whatever the descriptors say (the clamp of sbe_delivery_keys and sbe_commit_kernel).
//
//   is_session_event   template 2, schema 111
//   is_acknowledgment  template 2, schema 1
//   is_topic_message   template 1 and schema 1 / 111, template 2 and schema 1, or a type that
//                      contains "ORDER" or "TopicMessage" (the list's CREATE_ORDER and UPDATE_ORDER
//                      contain ORDER)
//   is_order_message   is_topic_message and: a type that contains "ORDER", or a payload that
//                      contains order_details, token_pair, quantity, side or client_order_id
//
// The type and the topic are short and are read where they lie; the payload search runs over the
// tile's bytes staged into an LDS window, and only for the records the clauses before it left
// undecided: a tile without such a record stages nothing.

constexpr uint32_t kOsOverlap = 14;  // the longest needle (client_order_id, 15 bytes) less one

__device__ __forceinline__ bool os_lit(const uint8_t* p, const char* s, uint32_t k) {
    for (uint32_t j = 0; j < k; ++j)
        if (p[j] != (uint8_t)s[j]) return false;
    return true;
}

// bit 0: [p, p + n) contains "ORDER" (the answer is then final: the other bit is not looked for);
// bit 1: it contains "TopicMessage"
__device__ inline uint32_t os_type_flags(const uint8_t* p, uint32_t n) {
    uint32_t f = 0;
    for (uint32_t i = 0; i + 5 <= n; ++i) {
        const uint8_t c = p[i];
        if (c == 'O' && os_lit(p + i + 1, "RDER", 4)) return 1u;
        if (c == 'T' && n - i >= 12 && os_lit(p + i + 1, "opicMessage", 11)) f = 2u;
    }
    return f;
}

// classify_topic: SBE_TC_ORDERS, SBE_TC_CONTROL or SBE_TC_UNKNOWN
__device__ inline uint32_t os_topic_class(const uint8_t* p, uint32_t n) {
    switch (n) {
        case 6: return os_lit(p, "orders", 6) ? SBE_TC_ORDERS : SBE_TC_UNKNOWN;
        case 19: return os_lit(p, "order_request_topic", 19) ? SBE_TC_ORDERS : SBE_TC_UNKNOWN;
        case 14: return os_lit(p, "_subscriptions", 14) ? SBE_TC_CONTROL : SBE_TC_UNKNOWN;
        case 4: return os_lit(p, "_ack", 4) ? SBE_TC_CONTROL : SBE_TC_UNKNOWN;
        case 8: return os_lit(p, "_control", 8) ? SBE_TC_CONTROL : SBE_TC_UNKNOWN;
        case 9: return os_lit(p, "_internal", 9) ? SBE_TC_CONTROL : SBE_TC_UNKNOWN;
        default: return SBE_TC_UNKNOWN;
    }
}

// The view that holds the record's payload bytes, or -1: no payload, or one without a needle.
__device__ __forceinline__ int os_payload_view(uint32_t st, uint32_t fl) {
    if (st == SBE_ST_TM || st == SBE_ST_SESSION_EVENT) return 3;
    if (st == SBE_ST_ACK && !(fl & SBE_FL_PAYLOAD_DEFAULT)) return 1;
    return -1;
}

// Everything the predicates say before the payload is read.  tpl / sch: hdr[1] / hdr[2] as decoded;
// [ty, ty + tyn): view 1 (read for SBE_ST_TM only); pln: length of the os_payload_view view (0
// without one).  need: SBE_PR_ORDER_MESSAGE hangs on the payload search.
__device__ inline uint32_t os_head(uint32_t st, uint32_t tpl, uint32_t sch, const uint8_t* ty, uint32_t tyn,
                                   uint32_t pln, bool& need) {
    need = false;
    if (st > SBE_ST_SESSION_EVENT && (st < SBE_ST_ERR_NULL_EMPTY || st > SBE_ST_ERR_ACK_SHORT)) return 0u;
    if (st >= SBE_ST_ERR_NULL_EMPTY && st != SBE_ST_ERR_UNKNOWN_TYPE) tpl = sch = 0;
    const uint32_t tf = st == SBE_ST_TM ? os_type_flags(ty, tyn) : 0u;
    uint32_t p = 0;
    if (tpl == SBE_SESSION_EVENT_TEMPLATE_ID && sch == SBE_CLUSTER_SCHEMA_ID) p |= SBE_PR_SESSION_EVENT;
    if (tpl == SBE_ACK_TEMPLATE_ID && sch == SBE_TOPIC_SCHEMA_ID) p |= SBE_PR_ACKNOWLEDGMENT | SBE_PR_TOPIC_MESSAGE;
    if (tpl == SBE_TM_TEMPLATE_ID && (sch == SBE_TOPIC_SCHEMA_ID || sch == SBE_CLUSTER_SCHEMA_ID)) p |= SBE_PR_TOPIC_MESSAGE;
    if (tf) p |= SBE_PR_TOPIC_MESSAGE;
    if (p & SBE_PR_TOPIC_MESSAGE) {
        if (tf & 1u) p |= SBE_PR_ORDER_MESSAGE;
        else need = st <= SBE_ST_SESSION_EVENT && pln != 0;
    }
    return p;
}

// 1..5: order_details, token_pair, quantity, side, client_order_id starts at p (15 readable bytes); 0: none
__device__ __forceinline__ uint32_t os_needle_at(uint32_t first, const uint8_t* p) {
    switch (first) {
        case 'o': return os_lit(p + 1, "rder_details", 12) ? 1u : 0u;
        case 't': return os_lit(p + 1, "oken_pair", 9) ? 2u : 0u;
        case 'q': return os_lit(p + 1, "uantity", 7) ? 3u : 0u;
        case 's': return os_lit(p + 1, "ide", 3) ? 4u : 0u;
        case 'c': return os_lit(p + 1, "lient_order_id", 14) ? 5u : 0u;
        default: return 0u;
    }
}
__device__ __forceinline__ uint32_t os_needle_len(uint32_t id) {  // 13, 10, 8, 4, 15
    return (uint32_t)((0x0f04080a0d00ull >> (8 * id)) & 0xffu);
}

// chunk c of the staged window: nibble j = the needle that starts at byte 16 c + j (it may run into
// the next chunk: the window has 16 spare bytes)
__device__ inline uint64_t os_chunk_hits(const uint8_t* win, uint32_t c) {
    const uint8_t* p = win + 16 * c;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    const uint32_t w[4] = {q[0], q[1], q[2], q[3]};
    uint64_t h = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) h |= (uint64_t)os_needle_at((w[j >> 2] >> (8 * (j & 3))) & 0xffu, p + j) << (4 * j);
    return h;
}

// a needle wholly inside the window bytes [a0, a1)?
__device__ inline bool os_range_hit(const uint64_t* hits, uint32_t a0, uint32_t a1) {
    if (a1 <= a0) return false;
    for (uint32_t c = a0 >> 4; c <= (a1 - 1) >> 4; ++c) {
        uint64_t h = hits[c];
        for (uint32_t p = 16 * c; h; h >>= 4, ++p) {
            const uint32_t id = (uint32_t)(h & 15u);
            if (id && p >= a0 && p + os_needle_len(id) <= a1) return true;
        }
    }
    return false;
}

// One round of one record's search, in window coordinates: the window holds the bytes [0, nbytes),
// the part of the view not yet searched is [c0, e0).  True: a needle lies inside the view.  False:
// c0 has moved on, to e0 when the view is done, else back from the window's end by the overlap (a
// needle that starts in the last bytes of this window is found whole in the next one); a view that
// starts in or behind those last bytes waits for a later window.
__device__ inline bool os_round(const uint64_t* hits, uint32_t nbytes, uint64_t& c0, uint64_t e0) {
    if (c0 >= nbytes) return false;
    const uint32_t stop = e0 < nbytes ? (uint32_t)e0 : nbytes;
    if (os_range_hit(hits, (uint32_t)c0, stop)) return true;
    if (e0 <= nbytes) c0 = e0;
    else if (c0 + kOsOverlap < nbytes) c0 = nbytes - kOsOverlap;
    return false;
}

#ifndef SEQNUM_HOST_CHECK  // tests/select/select_host_check.cpp compiles the code above for the host
struct OsArgs {
    const uint8_t* in;
    const uint64_t* rec_off;
    uint64_t n;
    const uint8_t* status;
    const uint8_t* flags;
    const uint16_t* hdr;
    const uint32_t* view_off;
    const uint32_t* view_len;
    uint8_t* pred;
    uint8_t* select;       // or null
    uint8_t* topic_class;  // or null
    uint64_t* totals;
};

constexpr uint32_t kOsWin = 16384;  // LDS window of a tile, bytes

// One wave per 64-record tile, one lane per record (the shape of sbe_commit_kernel).
__global__ __launch_bounds__(kWave) void sbe_order_select_kernel(OsArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kOsWin + 16];
    __shared__ uint64_t hits[kOsWin / 16];
    const int lane = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile, r = t0 + lane;
    const bool valid = r < a.n;
    uint32_t st = 0xff, pred = 0, tc = SBE_TC_UNKNOWN;
    uint64_t cur = 0, end = 0;  // the payload bytes not yet searched, as offsets into `in`
    bool pending = false;
    if (valid) {
        const uint64_t b = a.rec_off[r], e = a.rec_off[r + 1];
        const uint64_t L64 = e > b ? e - b : 0;
        const uint32_t L = L64 > 0xffffffffull ? 0xffffffffu : (uint32_t)L64;
        st = a.status[r];
        // view k, kept inside the record whatever the descriptors say
        auto view = [&](int k, uint32_t& o, uint32_t& l) {
            const uint32_t vo = a.view_off[5 * r + k], vl = a.view_len[5 * r + k];
            o = vo <= L ? vo : L;
            l = vl <= L - o ? vl : L - o;
        };
        uint32_t tyo = 0, tyn = 0, plo = 0, pln = 0;
        if (st == SBE_ST_TM) view(1, tyo, tyn);
        const int pv = os_payload_view(st, a.flags[r]);
        if (pv >= 0) view(pv, plo, pln);
        pred = os_head(st, a.hdr[4 * r + 1], a.hdr[4 * r + 2], a.in + b + tyo, tyn, pln, pending);
        if (st == SBE_ST_TM && a.topic_class) {
            uint32_t o, l;
            view(0, o, l);
            tc = os_topic_class(a.in + b + o, l);
        }
        cur = b + plo;
        end = cur + pln;
    }
    // rounds: the window starts at the first byte some lane still has to search
    while (__ballot(pending)) {
        const uint64_t ws = cm_wave_min64(pending ? cur : ~0ull), we = cm_wave_max64(pending ? end : 0ull);
        const uint8_t* p0 = a.in + ws;
        const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(p0) & 15u);
        const uint8_t* base = p0 - lead;  // 16-B aligned; every chunk read below holds a byte of [ws, we)
        const uint64_t span = (uint64_t)lead + (we - ws);
        const uint32_t nbytes = span < kOsWin ? (uint32_t)span : kOsWin;
        const uint32_t nch = (nbytes + 15) >> 4;
        typedef uint32_t os_u32x4 __attribute__((ext_vector_type(4)));
        for (uint32_t c = lane; c < nch; c += kWave)
            *reinterpret_cast<os_u32x4*>(win + 16 * c) =
                __builtin_nontemporal_load(reinterpret_cast<const os_u32x4*>(base) + c);
        if (lane == 0) *reinterpret_cast<uint4*>(win + 16 * nch) = make_uint4(0, 0, 0, 0);
        __syncthreads();
        for (uint32_t c = lane; c < nch; c += kWave) hits[c] = os_chunk_hits(win, c);
        __syncthreads();
        if (pending) {
            uint64_t c0 = (uint64_t)lead + (cur - ws);
            if (os_round(hits, nbytes, c0, (uint64_t)lead + (end - ws))) {
                pred |= SBE_PR_ORDER_MESSAGE;
                pending = false;
            } else {
                cur = ws + (c0 - lead);
                pending = cur < end;
            }
        }
        __syncthreads();
    }
    const bool order = valid && (pred & SBE_PR_ORDER_MESSAGE);
    const bool sel = order && st == SBE_ST_TM;
    if (valid) {
        a.pred[r] = (uint8_t)pred;
        if (a.select) a.select[r] = sel ? 1 : 0;
        if (a.topic_class) a.topic_class[r] = (uint8_t)tc;
    }
    const uint64_t ms = __ballot(sel), mo = __ballot(order);
    if (lane == 0) {
        if (ms) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals), (unsigned long long)__popcll(ms));
        if (mo) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals + 1), (unsigned long long)__popcll(mo));
    }
}
#endif
