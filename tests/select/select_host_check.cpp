// TEST ONLY: the device search of csrc/order_select.hpp (the type and topic tests, the chunk hits,
// the range test and the round rule) compiled for the host, so the CPU suite can run its logic
// against the model of tests/select_lib.py without a GPU.  The tile loop below restates the one of
// sbe_order_select_kernel with the wave operations written as loops over the 64 lanes and the
// window size and the address alignment of `in` as parameters, so that small windows put every
// needle across a window edge; the kernel's own staging is GPU-only and is checked by
// tests/test_gpu_order_select.py.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/sbecodec.h"

#define SEQNUM_HOST_CHECK 1
#define __device__
#define __forceinline__ inline
namespace {
#include "../../aeron-cluster-client-cpp_amd/csrc/order_select.hpp"
}  // namespace

// The arguments of sbe_order_select in host memory.  window: bytes of the staged window, a multiple
// of 16, at least 48; base_lead: the address of in[0] mod 16.  select / topic_class may be null.
extern "C" int chk_select(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const uint8_t* status,
                          const uint8_t* flags, const uint16_t* hdr, const uint32_t* view_off, const uint32_t* view_len,
                          uint32_t window, uint32_t base_lead, uint8_t* pred, uint8_t* select, uint8_t* topic_class,
                          uint64_t* totals) {
    if (window < 48 || window % 16 || base_lead > 15) return SBE_EINVAL;
    totals[0] = totals[1] = 0;
    const uint64_t total = n ? rec_off[n] : 0;  // bytes of `in` that may be read
    std::vector<uint64_t> win64((window + 16) / 8 + 1), hits(window / 16);
    uint8_t* win = reinterpret_cast<uint8_t*>(win64.data());
    for (uint64_t t0 = 0; t0 < n; t0 += 64) {
        const uint32_t lanes = (uint32_t)(n - t0 < 64 ? n - t0 : 64);
        uint32_t st[64], pr[64], tc[64];
        uint64_t cur[64], end[64];
        bool pending[64];
        for (uint32_t lane = 0; lane < lanes; ++lane) {
            const uint64_t r = t0 + lane;
            const uint64_t b = rec_off[r], e = rec_off[r + 1];
            const uint64_t L64 = e > b ? e - b : 0;
            const uint32_t L = L64 > 0xffffffffull ? 0xffffffffu : (uint32_t)L64;
            st[lane] = status[r];
            auto view = [&](int k, uint32_t& o, uint32_t& l) {
                const uint32_t vo = view_off[5 * r + k], vl = view_len[5 * r + k];
                o = vo <= L ? vo : L;
                l = vl <= L - o ? vl : L - o;
            };
            uint32_t tyo = 0, tyn = 0, plo = 0, pln = 0;
            if (st[lane] == SBE_ST_TM) view(1, tyo, tyn);
            const int pv = os_payload_view(st[lane], flags[r]);
            if (pv >= 0) view(pv, plo, pln);
            pr[lane] = os_head(st[lane], hdr[4 * r + 1], hdr[4 * r + 2], in + b + tyo, tyn, pln, pending[lane]);
            tc[lane] = SBE_TC_UNKNOWN;
            if (st[lane] == SBE_ST_TM) {
                uint32_t o, l;
                view(0, o, l);
                tc[lane] = os_topic_class(in + b + o, l);
            }
            cur[lane] = b + plo;
            end[lane] = cur[lane] + pln;
        }
        for (;;) {
            uint64_t ws = ~0ull, we = 0;
            bool any = false;
            for (uint32_t lane = 0; lane < lanes; ++lane)
                if (pending[lane]) {
                    any = true;
                    ws = cur[lane] < ws ? cur[lane] : ws;
                    we = end[lane] > we ? end[lane] : we;
                }
            if (!any) break;
            const uint32_t lead = (uint32_t)((base_lead + ws) & 15u);
            const uint64_t span = (uint64_t)lead + (we - ws);
            const uint32_t nbytes = span < window ? (uint32_t)span : window;
            const uint32_t nch = (nbytes + 15) >> 4;
            // whole 16-byte chunks from the aligned address below in + ws; what lies outside `in` reads 0 here
            for (uint32_t x = 0; x < 16 * nch; ++x) {
                const int64_t src = (int64_t)ws - lead + x;
                win[x] = src >= 0 && (uint64_t)src < total ? in[src] : 0;
            }
            std::memset(win + 16 * nch, 0, 16);
            for (uint32_t c = 0; c < nch; ++c) hits[c] = os_chunk_hits(win, c);
            for (uint32_t lane = 0; lane < lanes; ++lane) {
                if (!pending[lane]) continue;
                uint64_t c0 = (uint64_t)lead + (cur[lane] - ws);
                if (os_round(hits.data(), nbytes, c0, (uint64_t)lead + (end[lane] - ws))) {
                    pr[lane] |= SBE_PR_ORDER_MESSAGE;
                    pending[lane] = false;
                } else {
                    cur[lane] = ws + (c0 - lead);
                    pending[lane] = cur[lane] < end[lane];
                }
            }
        }
        for (uint32_t lane = 0; lane < lanes; ++lane) {
            const uint64_t r = t0 + lane;
            const bool order = (pr[lane] & SBE_PR_ORDER_MESSAGE) != 0, sel = order && st[lane] == SBE_ST_TM;
            pred[r] = (uint8_t)pr[lane];
            if (select) select[r] = sel ? 1 : 0;
            if (topic_class) topic_class[r] = (uint8_t)tc[lane];
            totals[0] += sel;
            totals[1] += order;
        }
    }
    return SBE_OK;
}
