// TEST ONLY: the per-record sizing and writing functions of csrc/commit_emit.hpp (ce_size_one,
// ce_frame) compiled for the host and driven as the two launches drive them, so that the CPU suite
// can check them against the composition in tests/commitsend_lib.py without a GPU.  The product
// runs them only inside commit_emit_measure / commit_emit_write; the block scans, the LDS window
// and the coalesced stores of those kernels are GPU-only (tests/test_gpu_commit_emit.py).
#include <cstdint>

#include "../../include/sbecodec.h"

#define COMMIT_EMIT_HOST_CHECK 1
#define __device__
#define __forceinline__ inline
namespace {
#include "../../aeron-cluster-client-cpp_amd/csrc/commit_emit.hpp"

struct ByteSink {
    uint8_t* p;
    uint64_t n = 0;
    void put(uint8_t b) { p[n++] = b; }
};
}  // namespace

// The arguments of sbe_emit_commit_offsets in host memory (dec and plan spelled out).
extern "C" int chk_emit(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const uint8_t* status,
                        const uint8_t* flags, const uint32_t* view_off, const uint32_t* view_len,
                        const uint64_t* seq, const uint8_t* cm, const uint32_t* tidx, const uint64_t* last,
                        const uint32_t* topic_id, const uint8_t* iarena, const uint32_t* ioff, uint32_t k,
                        const uint8_t* mask, uint32_t flg, int session, int64_t term, int64_t sess, uint8_t* out,
                        uint64_t cap, uint64_t* out_off, uint8_t* st, uint64_t* emit_idx, uint64_t* totals) {
    if ((flg & ~SBE_CE_LAST_ONLY) || ((flg & SBE_CE_LAST_ONLY) && mask) || k == 0 || k > SBE_COMMIT_MAX_TOPICS)
        return SBE_EINVAL;
    const CeIn a{in,   rec_off,  status, flags, view_off, view_len, seq, cm,  tidx,
                 last, topic_id, iarena, ioff,  k,        mask,     flg, (uint32_t)session, term, sess};
    uint64_t o = 0, m = 0, host = 0;
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t len;
        st[i] = (uint8_t)ce_size_one(a, i, len);
        host += st[i] == SBE_CE_HOST;
        out_off[i] = o;
        if (len) {
            emit_idx[m++] = i;
            if (o + len <= cap) {
                ByteSink s{out + o};
                ce_frame(s, a, ce_fields(a, i), [](ByteSink& t, const uint8_t* p, uint32_t c) {
                    for (uint32_t j = 0; j < c; ++j) t.put(p[j]);
                });
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
