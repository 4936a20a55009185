// TEST ONLY: the per-record functions of csrc/commit_fallback.hpp (cf_record, cf_size_one,
// cf_frame, with ce_size_one / ce_frame of csrc/commit_emit.hpp under them) compiled for the host
// and driven as the two launches drive them, so that the CPU suite can check the selection, the
// length rule (u16 wrap, the 1040-byte bound) and the frame composition with its clipping sink
// against the composition in tests/commitfallback_lib.py without a GPU.  The quoting helper
// (oj::quoted) and the decimal writer use device intrinsics and are checked on the GPU only
// (tests/test_gpu_commit_fallback.py); here a plain restatement of valueToQuotedStringN stands in
// for them.  The block scans, the LDS window and the coalesced stores are GPU-only as well.
#include <cstddef>
#include <cstdint>

#include "../../include/sbecodec.h"

#define COMMIT_EMIT_HOST_CHECK 1
#define __device__
#define __forceinline__ inline
namespace {
#include "../../aeron-cluster-client-cpp_amd/csrc/commit_emit.hpp"
#include "../../aeron-cluster-client-cpp_amd/csrc/commit_fallback.hpp"

struct ByteSink {
    uint8_t* p;
    uint64_t n = 0, left = ~0ull;
    void put(uint8_t b) {
        if (!left) return;
        if (p) p[n] = b;
        ++n;
        --left;
    }
};

void hex4(ByteSink& s, uint32_t v) {
    const char* hx = "0123456789abcdef";
    s.put('\\');
    s.put('u');
    for (int sh = 12; sh >= 0; sh -= 4) s.put((uint8_t)hx[(v >> sh) & 15]);
}
// jsoncpp valueToQuotedStringN(p, n, emitUTF8 = false), utf8ToCodepoint included
void quote(ByteSink& s, const uint8_t* p, uint32_t n) {
    s.put('"');
    for (uint32_t i = 0; i < n;) {
        const uint32_t c = p[i], left = n - i;
        switch (c) {
            case '"': s.put('\\'); s.put('"'); ++i; continue;
            case '\\': s.put('\\'); s.put('\\'); ++i; continue;
            case '\b': s.put('\\'); s.put('b'); ++i; continue;
            case '\f': s.put('\\'); s.put('f'); ++i; continue;
            case '\n': s.put('\\'); s.put('n'); ++i; continue;
            case '\r': s.put('\\'); s.put('r'); ++i; continue;
            case '\t': s.put('\\'); s.put('t'); ++i; continue;
            default: break;
        }
        if (c >= 0x20 && c < 0x80) {
            s.put((uint8_t)c);
            ++i;
            continue;
        }
        uint32_t cp = 0xFFFD, used = 1;
        if (c < 0x20) {
            cp = c;
        } else if (c < 0xE0) {
            if (left >= 2) {
                cp = ((c & 0x1F) << 6) | (p[i + 1] & 0x3F);
                used = 2;
                if (cp < 0x80) cp = 0xFFFD;
            }
        } else if (c < 0xF0) {
            if (left >= 3) {
                cp = ((c & 0x0F) << 12) | ((p[i + 1] & 0x3Fu) << 6) | (p[i + 2] & 0x3F);
                used = 3;
                if ((cp >= 0xD800 && cp <= 0xDFFF) || cp < 0x800) cp = 0xFFFD;
            }
        } else if (c < 0xF8) {
            if (left >= 4) {
                cp = ((c & 0x07) << 18) | ((p[i + 1] & 0x3Fu) << 12) | ((p[i + 2] & 0x3Fu) << 6) | (p[i + 3] & 0x3F);
                used = 4;
                if (cp < 0x10000) cp = 0xFFFD;
            }
        }
        i += used;
        if (cp < 0x10000) {
            hex4(s, cp);
        } else {
            cp -= 0x10000;
            hex4(s, 0xD800 + ((cp >> 10) & 0x3FF));
            hex4(s, 0xDC00 + (cp & 0x3FF));
        }
    }
    s.put('"');
}
void dec(ByteSink& s, uint64_t v) {
    char d[20];
    int c = 0;
    do d[c++] = (char)('0' + v % 10);
    while (v /= 10);
    while (c) s.put((uint8_t)d[--c]);
}
void copy(ByteSink& t, const uint8_t* p, uint32_t c) {
    for (uint32_t j = 0; j < c; ++j) t.put(p[j]);
}
}  // namespace

// The arguments of sbe_emit_commit_offsets_ex in host memory (dec, plan and fb spelled out).
extern "C" int chk_emit_fb(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const uint8_t* status,
                           const uint8_t* flags, const uint32_t* view_off, const uint32_t* view_len,
                           const uint64_t* seq, const uint64_t* ts, const uint8_t* cm, const uint8_t* kind,
                           const uint32_t* tok_off, const uint32_t* tok_len, const uint32_t* tidx,
                           const uint64_t* last, const uint32_t* topic_id, const uint8_t* iarena,
                           const uint32_t* ioff, const uint8_t* tarena, const uint32_t* toff, uint32_t k,
                           const uint8_t* dident, uint32_t didentn, uint64_t now_ns, uint64_t uuid_ns,
                           const uint8_t* mask, uint32_t flg, int session, int64_t term, int64_t sess, uint8_t* out,
                           uint64_t cap, uint64_t* out_off, uint8_t* st, uint64_t* emit_idx, uint64_t* totals) {
    if ((flg & ~SBE_CE_LAST_ONLY) || ((flg & SBE_CE_LAST_ONLY) && mask) || k == 0 || k > SBE_COMMIT_MAX_TOPICS ||
        didentn > SBE_COMMIT_TABLE_BYTES)
        return SBE_EINVAL;
    const CeIn c{in,   rec_off,  status, flags, view_off, view_len, seq, cm,  tidx,
                 last, topic_id, iarena, ioff,  k,        mask,     flg, (uint32_t)session, term, sess};
    const CfIn a{c, ts, kind, tok_off, tok_len, tarena, toff, dident, didentn, now_ns, uuid_ns};
    uint64_t o = 0, m = 0, host = 0;
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t len;
        st[i] = (uint8_t)cf_size_one(a, i, len, [](const CfRec& r) {
            ByteSink cnt{nullptr};
            cf_text(cnt, r, quote, dec);
            return cnt.n;
        });
        host += st[i] == SBE_CE_HOST;
        out_off[i] = o;
        if (len) {
            emit_idx[m++] = i;
            if (o + len <= cap) {
                ByteSink s{out + o};
                s.left = len;
                if (st[i] == SBE_CE_EMITTED_JSON) {
                    cf_frame(s, a, cf_record(a, i), len, copy, quote, dec);
                } else if (tidx[i] < k) {
                    ce_frame(s, c, ce_fields(c, i), copy);
                } else {  // a Lite frame for a named token outside the table
                    ce_frame(s, c, cf_lite_fields(cf_record(a, i)), copy);
                }
                if (s.n != len) return -100;  // the sizing and the writing function disagree
            } else {
                st[i] = SBE_CE_OVERFLOW;
            }
        }
        o += len;
    }
    out_off[n] = o;
    totals[0] = m;
    totals[1] = o;
    totals[2] = host;
    return SBE_OK;
}
