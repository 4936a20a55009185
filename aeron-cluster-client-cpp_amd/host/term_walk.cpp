// term_walk: the poll of one Aeron image over a raw term-buffer block, on one host thread (the
// semantics are stated at sbe_term_scan in sbecodec.h).  A file of its own, with no device code, so
// that tests/term can build it into a plain host program under a sanitizer.
#include "aeron_cluster_amd.hpp"

#include <cstring>

#include "sbecodec.h"

namespace aeron_cluster {

TermFragments term_walk(const std::uint8_t* block, std::size_t len, std::size_t start, std::size_t limit) {
    if ((len & 31) || (start & 31) || start > len) throw std::invalid_argument("term_walk: block and start are multiples of 32");
    TermFragments t;
    t.frag_off.push_back(0);
    std::uint64_t offset = start;
    bool stopped = false;
    while (t.flags.size() < limit && offset < len) {
        std::int32_t L;
        std::memcpy(&L, block + offset, 4);
        if (L <= 0) t.stop = SBE_TERM_STOP_UNCOMMITTED;
        else if (L < 32) t.stop = SBE_TERM_STOP_SHORT;
        else if (offset + (((std::uint64_t)L + 31) & ~31ull) > len) t.stop = SBE_TERM_STOP_PARTIAL;
        else {
            const std::uint64_t frame = offset;
            offset += ((std::uint64_t)L + 31) & ~31ull;
            std::uint16_t type;
            std::memcpy(&type, block + frame + 6, 2);
            if (type != 0) {
                t.frag_src.push_back((std::uint32_t)frame);
                t.flags.push_back(block[frame + 5]);
                t.frag_off.push_back(t.frag_off.back() + (std::uint64_t)L - 32);
            }
            continue;
        }
        stopped = true;
        break;
    }
    if (!stopped) t.stop = t.flags.size() == limit ? SBE_TERM_STOP_LIMIT : SBE_TERM_STOP_END;
    t.next = offset;
    return t;
}

}  // namespace aeron_cluster
