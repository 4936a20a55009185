// commit_class.hpp — included by sbe_codec.hip inside its anonymous namespace, after seqnum.hpp.
//
// The second half of ClusterClient::handle_incoming_message (src/cluster_client.cpp:1198-1303)
// for a decoded batch: should_skip_auto_commit (:847-886), extract_topic_from_message (:756-806)
// and the commit test of :1251, per record, on the device (sbe_classify_commits).  The input is
// what sbe_decode_batch(SBE_DEC_PARSE_MESSAGE) wrote for the same in / rec_off.
//
// Per record, in the reference's order (the first clause that fires gives the code):
//   status >= 16                                  SBE_CM_NOT_PARSED   (result.success false)
//   message_type is one of the six literals       SBE_CM_SKIP_TYPE    (:849-854)
//   message_id starts with "ack_"                 SBE_CM_SKIP_ACK_ID  (:859)
//   topic is "_ack" / "_subscriptions"            SBE_CM_SKIP_TOPIC   (:865)
//   topic is "_control", type is not REPLAY_COMPLETE and the payload does not contain it
//                                                 SBE_CM_SKIP_CONTROL (:871-878; a REPLAY_COMPLETE
//                                                 returns "not skipped" before the next clause)
//   payload empty                                 SBE_CM_SKIP_EMPTY_PAYLOAD (:881)
//   message_id empty                              SBE_CM_NO_ID        (:1251)
//   otherwise                                     SBE_CM_COMMIT
// SBE_ST_ACK records have message_type "Acknowledgment" (src/sbe_encoder.cpp:921): SKIP_TYPE.
// SBE_ST_SESSION_EVENT records never set message_id, so they never commit: they get SBE_CM_NO_ID
// whatever should_skip_auto_commit returns for them (its value cannot be observed there), with no
// topic extraction.  TM records: message_type view 1, message_id view 2, payload view 3, headers
// view 4 ("" under SBE_FL_HEADERS_E100).
//
// The topic (extract_topic_from_message) follows Json::parseFromStream with builder defaults, the
// call of the _sequence_number path: the rules in the header of seqnum.hpp apply unchanged (the
// whole root must parse, what follows it is ignored, a later duplicate key replaces the earlier
// one).  Headers, if not empty: a parsed object root with a member "topic" of scalar value gives
// the topic (a container value makes asString throw; that, a parse failure, a missing member, a
// null root and a non-object root, where isMember throws, all move on).  Payload, if not empty:
// a parsed object root with a member "topic" gives it (container: asString throws, fallback,
// "message" is not tried); else "message" an object with a member "topic" gives it (container:
// fallback); everything else is the fallback, table entry 0.
//
// A source that contains neither the bytes "topic" nor a backslash cannot hold a member named
// topic under any parse verdict, so it is not read as JSON: the kernel finds both needles over the
// staged 16-byte chunks, all lanes in parallel, and only the lanes of flagged records call the
// reader below (out of line, like json_seq_eval_call, so the common path keeps few registers).

enum : uint32_t { kCmKindContainer = 7 };  // internal: asString throws

// 1: one of the six auto-commit skip literals; 2: "REPLAY_COMPLETE"; 0: anything else
__device__ __forceinline__ bool cm_lit(const uint8_t* p, const char* s, uint32_t k) {
    for (uint32_t j = 0; j < k; ++j)
        if (p[j] != (uint8_t)s[j]) return false;
    return true;
}
__device__ __forceinline__ uint32_t cm_type_code(const uint8_t* p, uint32_t n) {
    switch (n) {
        case 9: return cm_lit(p, "SUBSCRIBE", 9) ? 1u : 0u;
        case 14: return ((p[0] == 'a' || p[0] == 'A') && cm_lit(p + 1, "cknowledgment", 13)) ? 1u : 0u;
        case 15: return cm_lit(p, "COMMIT_RESPONSE", 15) ? 1u : (cm_lit(p, "REPLAY_COMPLETE", 15) ? 2u : 0u);
        case 21: return ((p[0] == 'a' || p[0] == 'A') && cm_lit(p + 1, "cknowledgment_legacy", 20)) ? 1u : 0u;
        default: return 0u;
    }
}
// 1 "_ack", 2 "_subscriptions", 3 "_control", 0 other
__device__ __forceinline__ uint32_t cm_ctl_name(const uint8_t* p, uint32_t n) {
    if (n == 4) return cm_lit(p, "_ack", 4) ? 1u : 0u;
    if (n == 14) return cm_lit(p, "_subscriptions", 14) ? 2u : 0u;
    if (n == 8) return cm_lit(p, "_control", 8) ? 3u : 0u;
    return 0u;
}
// does [p, p+n) contain the bytes "topic" or a backslash (a candidate for the reader)?
__device__ inline bool cm_scan(const uint8_t* p, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t c = p[i];
        if (c == '\\') return true;
        if (c == 't' && n - i >= 5 && cm_lit(p + i + 1, "opic", 4)) return true;
    }
    return false;
}
__device__ inline bool cm_find_replay(const uint8_t* p, uint32_t n) {  // payload.find("REPLAY_COMPLETE")
    for (uint32_t i = 0; i + 15 <= n; ++i)
        if (p[i] == 'R' && cm_lit(p + i + 1, "EPLAY_COMPLETE", 14)) return true;
    return false;
}

// member name: "topic" or "message"?
struct CmKeySink {
    uint32_t len = 0;
    bool top = true, msg = true;
    __device__ __forceinline__ void put(uint32_t ch) {
        constexpr uint64_t kT = 0x0000006369706f74ull, kM = 0x006567617373656dull;  // "topic", "message"
        top = top && len < 5 && ch == (uint32_t)((kT >> (8 * (len & 7))) & 0xff);
        msg = msg && len < 7 && ch == (uint32_t)((kM >> (8 * (len & 7))) & 0xff);
        ++len;
    }
};
// decoded string == ref[0, n)?
struct CmEqSink {
    const uint8_t* ref;
    uint32_t n, i = 0;
    bool eq = true;
    __device__ __forceinline__ void put(uint32_t ch) {
        eq = eq && i < n && ref[i] == (uint8_t)ch;
        ++i;
    }
    __device__ __forceinline__ bool equal() const { return eq && i == n; }
};

// What one document says about "topic": kinds 0 = no such member, SBE_TOPIC_KIND_* or
// kCmKindContainer; [s, e) the token (strings: between the quotes), relative to the document.
struct CmDoc {
    bool ok = false, root_obj = false, msg_obj = false;
    uint32_t rk = 0, rs = 0, re = 0;  // root.topic
    uint32_t mk = 0, ms = 0, me = 0;  // root.message.topic (msg_obj: root.message is an object)
};

// The document walk of json_seq_eval (same tokens, same grammar, same failures) with another
// question asked of it.  d.ok false: parseFromStream returned false or threw.
__device__ void cm_doc_eval(const uint8_t* p, uint32_t n, CmDoc& d) {
    JCur c{p, n, 0};
    if (n >= 3 && p[0] == 0xEF && p[1] == 0xBB && p[2] == 0xBF) c.i = 3;  // skipBom
    uint64_t kind_bits[(kJsonStackLimit + 63) / 64];  // 1: object, 0: array, per open container
    int depth = 0;
    bool in_msg = false;  // the container at depth 2 is root.message, an object
    int pend = 0;         // member whose value comes next: 1 root.topic, 2 root.message, 3 root.message.topic
    uint32_t s, e;
    int t;
    enum { S_VALUE, S_KEY, S_OAFTER, S_AFIRST, S_AAFTER } st = S_VALUE;
    auto is_obj = [&](int dd) { return (kind_bits[dd >> 6] >> (dd & 63)) & 1; };
    auto push = [&](bool obj) {
        const uint64_t b = 1ull << (depth & 63);
        kind_bits[depth >> 6] = obj ? (kind_bits[depth >> 6] | b) : (kind_bits[depth >> 6] & ~b);
        ++depth;
    };
    auto set = [&](int what, uint32_t kind, uint32_t ts, uint32_t te) {
        if (what == 1) {
            d.rk = kind;
            d.rs = ts;
            d.re = te;
        } else if (what == 3) {
            d.mk = kind;
            d.ms = ts;
            d.me = te;
        }
    };
    for (;;) {
        bool value_done = false;
        if (st == S_VALUE || st == S_AFIRST) {
            if (st == S_AFIRST) {  // readArray: ']' right after '[' or ',' (spaces only)
                c.skip_spaces();
                if (c.i < c.n && c.p[c.i] == ']') {
                    ++c.i;
                    --depth;
                    value_done = true;
                }
            }
            if (!value_done) {
                if (depth >= kJsonStackLimit) return;  // "Exceeded stackLimit in readValue()" (thrown)
                do t = jtoken(c, s, e);
                while (t == JT_COMMENT);
                const int what = pend;
                pend = 0;
                if (t == JT_OBEG) {
                    push(true);
                    if (depth == 1) d.root_obj = true;
                    if (what == 2) {
                        d.msg_obj = true;
                        in_msg = true;
                    }
                    set(what, kCmKindContainer, 0, 0);
                    st = S_KEY;
                    continue;
                }
                if (t == JT_ABEG) {
                    push(false);
                    set(what, kCmKindContainer, 0, 0);
                    st = S_AFIRST;
                    continue;
                }
                if (t == JT_NUM) {
                    uint64_t v;
                    if (!jnum_seq(p, s, e, v)) return;
                    set(what, SBE_TOPIC_KIND_NUMBER, s, e);
                } else if (t == JT_STR) {
                    NullSink k;
                    if (!jdecode_string(p, s, e, k)) return;
                    if (what) {
                        bool esc = false;
                        for (uint32_t j = s + 1; j + 1 < e; ++j) esc = esc || p[j] == '\\';
                        set(what, esc ? SBE_TOPIC_KIND_STRING_ESC : SBE_TOPIC_KIND_STRING, s + 1, e - 1);
                    }
                } else if (t == JT_LIT) {
                    set(what, p[s] == 't' ? SBE_TOPIC_KIND_TRUE : p[s] == 'f' ? SBE_TOPIC_KIND_FALSE : SBE_TOPIC_KIND_NULL,
                        s, e);
                } else {
                    return;  // "Syntax error: value, object or array expected."
                }
                value_done = true;
            }
        } else if (st == S_KEY) {  // member name, or '}' (empty object / trailing comma)
            do t = jtoken(c, s, e);
            while (t == JT_COMMENT);
            if (t == JT_OEND) {
                if (depth == 2) in_msg = false;
                --depth;
                value_done = true;
            } else {
                if (t != JT_STR) return;
                CmKeySink k;
                if (!jdecode_string(p, s, e, k)) return;
                if (depth == 1 && d.root_obj) {
                    if (k.top && k.len == 5) {
                        pend = 1;
                    } else if (k.msg && k.len == 7) {  // the member is replaced
                        pend = 2;
                        d.msg_obj = false;
                        d.mk = 0;
                    }
                } else if (depth == 2 && in_msg && k.top && k.len == 5) {
                    pend = 3;
                }
                if (jtoken(c, s, e) != JT_COLON) return;  // "Missing ':' after object member name"
                st = S_VALUE;
                continue;
            }
        } else if (st == S_OAFTER) {  // ',' or '}'; after comments, the next token stands as separator
            t = jtoken(c, s, e);
            if (t != JT_OEND && t != JT_COMMA && t != JT_COMMENT) return;  // "Missing ',' or '}' ..."
            while (t == JT_COMMENT) t = jtoken(c, s, e);
            if (t == JT_OEND) {
                if (depth == 2) in_msg = false;
                --depth;
                value_done = true;
            } else {
                st = S_KEY;
                continue;
            }
        } else {  // S_AAFTER
            do t = jtoken(c, s, e);
            while (t == JT_COMMENT);
            if (t == JT_AEND) {
                --depth;
                value_done = true;
            } else {
                if (t != JT_COMMA) return;  // "Missing ',' or ']' in array declaration"
                st = S_AFIRST;
                continue;
            }
        }
        if (value_done) {
            if (depth == 0) break;  // the root is complete; what follows is ignored
            st = is_obj(depth - 1) ? S_OAFTER : S_AAFTER;
        }
    }
    d.ok = true;
}

// One TM record as the classifier sees it: flat pointers (LDS window or HBM) to the four views.
struct CmRec {
    const uint8_t *ty, *id, *pl, *hd;
    uint32_t tyn, idn, pln, hdn;
    uint32_t ploff, hdoff;  // view offsets inside the record (for topic_off)
    bool plc, hdc;          // cm_scan of payload / headers
};
struct CmTable {
    const uint8_t* arena;
    const uint32_t* off;  // [k + 1], clamped to SBE_COMMIT_TABLE_BYTES
    uint32_t k;
    __device__ __forceinline__ uint32_t len(uint32_t j) const { return off[j + 1] > off[j] ? off[j + 1] - off[j] : 0u; }
};
struct CmOut {
    uint32_t cm, src, kind, off, len, idx;
};

// extract_topic_from_message: src / kind / [off, off+len) relative to the record; tok: the token
__device__ void cm_extract(const CmRec& r, CmOut& o, const uint8_t*& tok) {
    o.src = SBE_TOPIC_SRC_FALLBACK;
    o.kind = SBE_TOPIC_KIND_NONE;
    o.off = o.len = 0;
    tok = nullptr;
    if (r.hdn && r.hdc) {
        CmDoc d;
        cm_doc_eval(r.hd, r.hdn, d);
        if (d.ok && d.root_obj && d.rk && d.rk != kCmKindContainer) {
            o.src = SBE_TOPIC_SRC_HEADERS;
            o.kind = d.rk;
            o.off = r.hdoff + d.rs;
            o.len = d.re - d.rs;
            tok = r.hd + d.rs;
            return;
        }
    }
    if (r.pln && r.plc) {
        CmDoc d;
        cm_doc_eval(r.pl, r.pln, d);
        if (!d.ok || !d.root_obj) return;
        uint32_t k = 0, s = 0, e = 0, src = 0;
        if (d.rk) {
            k = d.rk, s = d.rs, e = d.re, src = SBE_TOPIC_SRC_PAYLOAD;
        } else if (d.msg_obj && d.mk) {
            k = d.mk, s = d.ms, e = d.me, src = SBE_TOPIC_SRC_PAYLOAD_MESSAGE;
        }
        if (k && k != kCmKindContainer) {
            o.src = src;
            o.kind = k;
            o.off = r.ploff + s;
            o.len = e - s;
            tok = r.pl + s;
        }
    }
}

// decoded topic token == ref[0, n)?  (string kinds only)
__device__ bool cm_topic_eq(const uint8_t* tok, uint32_t len, uint32_t kind, const uint8_t* ref, uint32_t n) {
    if (kind == SBE_TOPIC_KIND_STRING) {
        if (len != n) return false;
        for (uint32_t j = 0; j < n; ++j)
            if (tok[j] != ref[j]) return false;
        return true;
    }
    CmEqSink k{ref, n};
    jdecode_string(tok - 1, 0, len + 2, k);  // the token with its quotes; it decoded once already
    return k.equal();
}

// The whole of one TM record.  fb_ctl: cm_ctl_name of the fallback topic (table entry 0).
__device__ void cm_classify(const CmRec& r, const CmTable& tb, uint32_t fb_ctl, CmOut& o) {
    o.src = SBE_TOPIC_SRC_NONE;
    o.kind = SBE_TOPIC_KIND_NONE;
    o.off = o.len = 0;
    o.idx = SBE_TOPIC_UNKNOWN;
    const uint32_t tc = cm_type_code(r.ty, r.tyn);
    if (tc == 1) {
        o.cm = SBE_CM_SKIP_TYPE;
        return;
    }
    if (r.idn >= 4 && cm_lit(r.id, "ack_", 4)) {
        o.cm = SBE_CM_SKIP_ACK_ID;
        return;
    }
    const uint8_t* tok;
    cm_extract(r, o, tok);
    const bool str = o.kind == SBE_TOPIC_KIND_STRING || o.kind == SBE_TOPIC_KIND_STRING_ESC;
    uint32_t ctl = 0;
    if (o.src == SBE_TOPIC_SRC_FALLBACK) {
        ctl = fb_ctl;
    } else if (str) {
        if (cm_topic_eq(tok, o.len, o.kind, reinterpret_cast<const uint8_t*>("_ack"), 4)) ctl = 1;
        else if (cm_topic_eq(tok, o.len, o.kind, reinterpret_cast<const uint8_t*>("_subscriptions"), 14)) ctl = 2;
        else if (cm_topic_eq(tok, o.len, o.kind, reinterpret_cast<const uint8_t*>("_control"), 8)) ctl = 3;
    }
    if (ctl == 1 || ctl == 2) {
        o.cm = SBE_CM_SKIP_TOPIC;
        return;
    }
    if (ctl == 3) {
        if (tc != 2 && !cm_find_replay(r.pl, r.pln)) {
            o.cm = SBE_CM_SKIP_CONTROL;
            return;
        }
    } else if (r.pln == 0) {
        o.cm = SBE_CM_SKIP_EMPTY_PAYLOAD;
        return;
    }
    if (r.idn == 0) {
        o.cm = SBE_CM_NO_ID;
        return;
    }
    o.cm = SBE_CM_COMMIT;
    if (o.src == SBE_TOPIC_SRC_FALLBACK) {
        o.idx = 0;
    } else if (!str) {
        o.idx = SBE_TOPIC_HOST;
    } else {
        for (uint32_t j = 0; j < tb.k; ++j)
            if (cm_topic_eq(tok, o.len, o.kind, tb.arena + tb.off[j], tb.len(j))) {
                o.idx = j;
                break;
            }
    }
}

#ifndef SEQNUM_HOST_CHECK  // tests/autocommit/commit_host_check.cpp compiles the code above for the host
__device__ __noinline__ void cm_classify_call(const CmRec& r, const CmTable& tb, uint32_t fb_ctl, CmOut& o) {
    cm_classify(r, tb, fb_ctl, o);
}

struct CmArgs {
    const uint8_t* in;
    const uint64_t* rec_off;
    uint64_t n;
    const uint8_t* status;
    const uint8_t* flags;
    const uint32_t* view_off;
    const uint32_t* view_len;
    const uint8_t* tarena;
    const uint32_t* toff;
    uint32_t k;
    uint8_t* cm;
    uint8_t* src;
    uint8_t* kind;
    uint32_t* off;
    uint32_t* len;
    uint32_t* idx;
    uint64_t* last;
    uint64_t* count;
};

// last = UINT64_MAX (none), count = 0: stream-ordered before the classify launch
__global__ __launch_bounds__(kWave) void sbe_commit_init(uint64_t* last, uint64_t* count, uint32_t k) {
    for (uint32_t j = threadIdx.x; j < k + 2; j += kWave) {
        if (j < k) last[j] = ~0ull;
        count[j] = 0;
    }
}

constexpr uint32_t kCmWin = 16384;                // LDS window of a tile, bytes
constexpr uint32_t kCmLong = kCmWin - 16;         // longer records are read from HBM
constexpr uint32_t kCmTopicLE = 0x69706f74u;      // "topi"

// chunk c of the staged window: bit j = "topic" starts at byte 16 c + j, bit 16 + j = byte 16 c + j
// is a backslash (the needle may run into the next chunk: the window has 16 spare bytes)
__device__ __forceinline__ uint32_t cm_chunk_hits(const uint8_t* win, uint32_t c) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(win + 16 * c);
    const uint4 v = *reinterpret_cast<const uint4*>(q);
    const uint32_t w[5] = {v.x, v.y, v.z, v.w, q[4]};
    // a needle that starts in this chunk has its 'p' in these 20 bytes: without a 'p' and without a
    // backslash (any-tests, exact as "some byte matches") the 16 exact alignments are not tried
    uint32_t pre = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint32_t x = w[j] ^ 0x70707070u;
        pre |= ((x - 0x01010101u) & ~x) | (j < 4 ? bs_any(w[j]) : 0u);
    }
    if (!(pre & 0x80808080u)) return 0u;
    uint32_t h = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t x = s ? __builtin_amdgcn_alignbyte(w[j + 1], w[j], s) : w[j];
            const uint32_t nx = (w[j + 1] >> (8 * s)) & 0xffu;
            h |= (x == kCmTopicLE && nx == 'c') ? 1u << (4 * j + s) : 0u;
        }
        const uint32_t b = bs_bytes_exact(w[j]);  // 0x80 per backslash byte
        h |= (((b >> 7) & 1u) | ((b >> 14) & 2u) | ((b >> 21) & 4u) | ((b >> 28) & 8u)) << (16 + 4 * j);
    }
    return h;
}
// a needle wholly inside, or a backslash inside, the window bytes [a0, a1)?
__device__ bool cm_range_hit(const uint32_t* hits, uint32_t a0, uint32_t a1) {
    if (a1 <= a0) return false;
    for (uint32_t c = a0 >> 4; c <= (a1 - 1) >> 4; ++c) {
        const uint32_t h = hits[c];
        if (!h) continue;
        const uint32_t base = 16 * c;
        for (uint32_t j = 0; j < 16; ++j) {
            const uint32_t p = base + j;
            if (p < a0) continue;
            if (((h >> (16 + j)) & 1u) && p < a1) return true;
            if (((h >> j) & 1u) && p + 5 <= a1) return true;
        }
    }
    return false;
}

__device__ __forceinline__ uint64_t cm_wave_min64(uint64_t v) {
    for (int d = 32; d; d >>= 1) {
        const uint64_t o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t cm_wave_max64(uint64_t v) {
    for (int d = 32; d; d >>= 1) {
        const uint64_t o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// One wave per 64-record tile, one lane per record.
__device__ __forceinline__ void cm_tile(const CmArgs& a) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kCmWin + 16];
    __shared__ uint32_t hits[kCmWin / 16];
    __shared__ uint32_t toff[SBE_COMMIT_MAX_TOPICS + 1];
    const int lane = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile, r = t0 + lane;
    const bool valid = r < a.n;
    for (uint32_t j = lane; j <= a.k; j += kWave) toff[j] = min(a.toff[j], (uint32_t)SBE_COMMIT_TABLE_BYTES);
    __syncthreads();
    const uint32_t fb_ctl = cm_ctl_name(a.tarena + toff[0], toff[1] > toff[0] ? toff[1] - toff[0] : 0u);

    uint64_t b = 0, e = 0;
    uint32_t st = 0xff, fl = 0, vo[4] = {0, 0, 0, 0}, vl[4] = {0, 0, 0, 0};
    if (valid) {
        b = a.rec_off[r];
        e = a.rec_off[r + 1];
        st = a.status[r];
    }
    const uint64_t L64 = e > b ? e - b : 0;
    const uint32_t L = L64 > 0xffffffffull ? 0xffffffffu : (uint32_t)L64;
    CmOut o{SBE_CM_NOT_PARSED, SBE_TOPIC_SRC_NONE, SBE_TOPIC_KIND_NONE, 0, 0, SBE_TOPIC_UNKNOWN};
    if (st == SBE_ST_ACK) o.cm = SBE_CM_SKIP_TYPE;
    if (st == SBE_ST_SESSION_EVENT) o.cm = SBE_CM_NO_ID;
    bool pending = valid && st == SBE_ST_TM;
    if (pending) {
        fl = a.flags[r];
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // views 1..4, kept inside the record whatever the descriptors say
            const uint32_t vo_k = a.view_off[5 * r + 1 + k], vl_k = a.view_len[5 * r + 1 + k];
            vo[k] = vo_k <= L ? vo_k : L;
            vl[k] = vl_k <= L - vo[k] ? vl_k : L - vo[k];
        }
        if (fl & SBE_FL_HEADERS_E100) vl[3] = 0;
    }
    // The out-of-line reader takes its record and result by reference, which puts them on the stack:
    // both are built inside the slow branch only, so that the fast path keeps its state in registers
    // (with `o` itself passed down, every lane wrote it to scratch: 78 MB a launch on 1 M records).
    auto run = [&](const uint8_t* rec, bool plc, bool hdc) {
        if (cm_type_code(rec + vo[0], vl[0]) == 1) {
            o.cm = SBE_CM_SKIP_TYPE;
        } else if (vl[1] >= 4 && cm_lit(rec + vo[1], "ack_", 4)) {
            o.cm = SBE_CM_SKIP_ACK_ID;
        } else if (!plc && !hdc && !fb_ctl) {  // no parse: the fallback topic, not a control name
            o.src = SBE_TOPIC_SRC_FALLBACK;
            o.cm = vl[2] == 0 ? SBE_CM_SKIP_EMPTY_PAYLOAD : vl[1] == 0 ? SBE_CM_NO_ID : SBE_CM_COMMIT;
            if (o.cm == SBE_CM_COMMIT) o.idx = 0;
        } else {
            const CmRec rc{rec + vo[0], rec + vo[1], rec + vo[2], rec + vo[3], vl[0], vl[1], vl[2], vl[3],
                           vo[2], vo[3], plc, hdc};
            const CmTable tb{a.tarena, toff, a.k};
            CmOut t;
            cm_classify_call(rc, tb, fb_ctl, t);
            o = t;
        }
    };
    // records longer than the window: read from HBM (as decode's long records are)
    if (pending && L > kCmLong) {
        const uint8_t* rec = a.in + b;
        run(rec, vl[2] ? cm_scan(rec + vo[2], vl[2]) : false, vl[3] ? cm_scan(rec + vo[3], vl[3]) : false);
        pending = false;
    }
    while (__ballot(pending)) {
        const uint64_t ws = cm_wave_min64(pending ? b : ~0ull), we = cm_wave_max64(pending ? e : 0ull);
        const uint8_t* p0 = a.in + ws;
        const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(p0) & 15u);
        const uint8_t* base = p0 - lead;  // 16-B aligned; every chunk read below holds a byte of [ws, we)
        const uint64_t span = (uint64_t)lead + (we - ws);
        const uint32_t nbytes = span < kCmWin ? (uint32_t)span : kCmWin;
        const uint32_t nch = (nbytes + 15) >> 4;
        typedef uint32_t cm_u32x4 __attribute__((ext_vector_type(4)));
        for (uint32_t c = lane; c < nch; c += kWave)
            *reinterpret_cast<cm_u32x4*>(win + 16 * c) =
                __builtin_nontemporal_load(reinterpret_cast<const cm_u32x4*>(base) + c);
        if (lane == 0) *reinterpret_cast<uint4*>(win + 16 * nch) = make_uint4(0, 0, 0, 0);
        __syncthreads();
        uint32_t any = 0;
        for (uint32_t c = lane; c < nch; c += kWave) {
            const uint32_t h = cm_chunk_hits(win, c);
            hits[c] = h;
            any |= h;
        }
        __syncthreads();
        const bool wave_any = __ballot(any != 0) != 0;
        const uint64_t o0 = (uint64_t)lead + (b - ws);
        if (pending && o0 + L <= nbytes) {
            const uint32_t w0 = (uint32_t)o0;
            bool plc = false, hdc = false;
            if (wave_any) {
                plc = cm_range_hit(hits, w0 + vo[2], w0 + vo[2] + vl[2]);
                hdc = cm_range_hit(hits, w0 + vo[3], w0 + vo[3] + vl[3]);
            }
            run(win + w0, plc, hdc);
            pending = false;
        }
        __syncthreads();
    }
    if (valid) {
        a.cm[r] = (uint8_t)o.cm;
        a.src[r] = (uint8_t)o.src;
        a.kind[r] = (uint8_t)o.kind;
        a.off[r] = o.off;
        a.len[r] = o.len;
        a.idx[r] = o.idx;
    }
    // last / count: reduced in the wave (ballots), one atomic per table entry per wave
    const bool com = valid && o.cm == SBE_CM_COMMIT;
    const uint32_t slot = o.idx == SBE_TOPIC_UNKNOWN ? a.k : o.idx == SBE_TOPIC_HOST ? a.k + 1 : o.idx;
    uint64_t todo = __ballot(com);
    while (todo) {
        const uint32_t s0 = __shfl((int)slot, __ffsll((long long)todo) - 1);
        const uint64_t m = __ballot(com && slot == s0);
        if (lane == 0) {
            atomicAdd(reinterpret_cast<unsigned long long*>(a.count + s0), (unsigned long long)__popcll(m));
            if (s0 < a.k)  // UINT64_MAX (none) is -1: a signed maximum
                __hip_atomic_fetch_max(reinterpret_cast<long long*>(a.last + s0), (long long)(t0 + 63 - __clzll((long long)m)),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        todo &= ~m;
    }
}
__global__ __launch_bounds__(kWave) void sbe_commit_kernel(CmArgs a) { cm_tile(a); }
// sbe_classify_commits_counted: a.n is the capacity the grid was laid out by; a tile past the count
// exits behind the load of the count.
__global__ __launch_bounds__(kWave) void sbe_commit_counted_kernel(CmArgs a, const uint64_t* n_dev) {
    a.n = counted_n(n_dev, a.n);
    if ((uint64_t)blockIdx.x * kTile >= a.n) return;
    cm_tile(a);
}
#endif
