// TEST ONLY: the trie builder and the document walk of csrc/json_paths.hpp (with the JSON reader
// of csrc/seqnum.hpp under them) compiled for the host, so the CPU suite can run their logic
// against the restatement in paths_ref.cpp without a GPU.  The product runs the walk only inside
// sbe_json_extract_kernel; the window staging and the LDS result rows of that kernel are GPU-only
// and are checked by tests/test_gpu_jsonpaths.py.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/sbecodec.h"

#define SEQNUM_HOST_CHECK 1
#define __device__
#define __forceinline__ inline
#define __constant__ static
namespace {
#include "../../aeron-cluster-client-cpp_amd/csrc/seqnum.hpp"
#include "../../aeron-cluster-client-cpp_amd/csrc/json_paths.hpp"
}  // namespace

// The arguments of sbe_json_extract_batch, in host memory (same signature as pref_extract, with
// the entry point's verdict on the path table: 0, or -1 for SBE_EINVAL with nothing written).
extern "C" int chk_extract(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const uint8_t* status,
                           const uint8_t* flags, const uint32_t* view_off, const uint32_t* view_len, uint32_t view,
                           const uint8_t* select, uint32_t n_paths, const uint8_t* depth, const uint8_t* names,
                           const uint32_t* name_off, uint8_t* doc, uint8_t* root_kind, uint8_t* kind, uint32_t* off,
                           uint32_t* len) {
    const sbe_json_paths ps{n_paths, depth, names, name_off};
    JxTrie T;
    if (!jx_build_trie(&ps, T)) return SBE_EINVAL;
    const uint32_t P = T.n_paths;
    for (uint64_t i = 0; i < n; ++i) {
        const JxRow row{kind + i * P, off + i * P, len + i * P};
        for (uint32_t p = 0; p < P; ++p) {
            row.kind[p] = SBE_JX_MISSING;
            row.off[p] = row.len[p] = 0;
        }
        doc[i] = SBE_JX_NOT_SELECTED;
        root_kind[i] = SBE_JX_MISSING;
        if ((select && !select[i]) || (status && status[i] != SBE_ST_TM)) continue;
        const uint64_t b = rec_off[i], e = rec_off[i + 1];
        const uint64_t L64 = e > b ? e - b : 0;
        const uint32_t L = L64 > 0xffffffffull ? 0xffffffffu : (uint32_t)L64;
        uint32_t vo = 0, dl = L;
        if (status) {
            const uint32_t o = view_off[5 * i + view], l = view_len[5 * i + view];
            vo = o <= L ? o : L;
            dl = l <= L - vo ? l : L - vo;
            if (view == 4 && (flags[i] & SBE_FL_HEADERS_E100)) dl = 0;
        }
        doc[i] = SBE_JX_EMPTY;
        if (!dl) continue;
        uint32_t rk = SBE_JX_MISSING;
        doc[i] = (uint8_t)jx_walk(in + b + vo, dl, T, row, vo, rk);
        root_kind[i] = (uint8_t)rk;
    }
    return SBE_OK;
}
