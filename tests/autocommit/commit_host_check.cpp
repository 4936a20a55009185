// TEST ONLY: the device classifier of csrc/commit_class.hpp (with the JSON reader of
// csrc/seqnum.hpp under it) compiled for the host, so the CPU suite can run its logic against the
// restatement in commit_ref.cpp without a GPU.  The product runs it only inside
// sbe_commit_kernel; the window staging and the chunk-parallel needle search of that kernel are
// GPU-only and are checked by tests/test_gpu_autocommit.py.
#include <cstdint>

#include "../../include/sbecodec.h"

#define SEQNUM_HOST_CHECK 1
#define __device__
#define __forceinline__ inline
#define __constant__ static
namespace {
#include "../../aeron-cluster-client-cpp_amd/csrc/seqnum.hpp"
#include "../../aeron-cluster-client-cpp_amd/csrc/commit_class.hpp"
}  // namespace

// The arguments of sbe_classify_commits, in host memory (same signature as cref_classify).
extern "C" void chk_classify(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const uint8_t* status,
                             const uint8_t* flags, const uint32_t* view_off, const uint32_t* view_len,
                             const uint8_t* tarena, const uint32_t* toff, uint32_t k, uint8_t* cm, uint8_t* src,
                             uint8_t* kind, uint32_t* off, uint32_t* len, uint32_t* idx, uint64_t* last,
                             uint64_t* count) {
    uint32_t ct[SBE_COMMIT_MAX_TOPICS + 1];
    for (uint32_t j = 0; j <= k; ++j) ct[j] = toff[j] < SBE_COMMIT_TABLE_BYTES ? toff[j] : SBE_COMMIT_TABLE_BYTES;
    const CmTable tb{tarena, ct, k};
    const uint32_t fb_ctl = cm_ctl_name(tarena + ct[0], tb.len(0));
    for (uint32_t j = 0; j < k; ++j) last[j] = ~0ull;
    for (uint32_t j = 0; j < k + 2; ++j) count[j] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        CmOut o{SBE_CM_NOT_PARSED, SBE_TOPIC_SRC_NONE, SBE_TOPIC_KIND_NONE, 0, 0, SBE_TOPIC_UNKNOWN};
        if (status[i] == SBE_ST_ACK) o.cm = SBE_CM_SKIP_TYPE;
        if (status[i] == SBE_ST_SESSION_EVENT) o.cm = SBE_CM_NO_ID;
        if (status[i] == SBE_ST_TM) {
            const uint8_t* rec = in + rec_off[i];
            const uint32_t* vo = view_off + 5 * i;
            const uint32_t* vl = view_len + 5 * i;
            const uint32_t hn = (flags[i] & SBE_FL_HEADERS_E100) ? 0 : vl[4];
            const CmRec r{rec + vo[1], rec + vo[2], rec + vo[3], rec + vo[4], vl[1], vl[2], vl[3], hn,
                          vo[3], vo[4], cm_scan(rec + vo[3], vl[3]), cm_scan(rec + vo[4], hn)};
            cm_classify(r, tb, fb_ctl, o);
        }
        cm[i] = (uint8_t)o.cm;
        src[i] = (uint8_t)o.src;
        kind[i] = (uint8_t)o.kind;
        off[i] = o.off;
        len[i] = o.len;
        idx[i] = o.idx;
        if (o.cm == SBE_CM_COMMIT) {
            const uint32_t slot = o.idx == SBE_TOPIC_UNKNOWN ? k : o.idx == SBE_TOPIC_HOST ? k + 1 : o.idx;
            ++count[slot];
            if (slot < k) last[slot] = i;
        }
    }
}
