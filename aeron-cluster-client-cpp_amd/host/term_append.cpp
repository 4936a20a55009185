// term_append: the offer loop of an exclusive publication over a batch of records into a raw
// term-buffer block, on one host thread (the semantics are stated at sbe_term_append in sbecodec.h).
// A file of its own, with no device code, so that tests/termappend can build it into a plain host
// program under a sanitizer.
#include "aeron_cluster_amd.hpp"

#include <cstring>

#include "sbecodec.h"

namespace aeron_cluster {

std::uint64_t term_frames_length(std::uint64_t len, std::uint32_t mtu) {
    const std::uint64_t maxp = mtu - 32u;
    if (len <= maxp) return (32 + len + 31) & ~31ull;
    const std::uint64_t rem = len % maxp;
    return (len / maxp) * mtu + (rem ? (32 + rem + 31) & ~31ull : 0);
}

namespace {
void put_header(std::uint8_t* at, std::uint32_t frame_length, std::uint8_t flags, std::uint16_t type, std::uint64_t offset,
                const TermHeader& h) {
    const std::int32_t w[6] = {(std::int32_t)frame_length, 0, (std::int32_t)((std::uint32_t)h.term_offset_base + (std::uint32_t)offset),
                               h.session_id, h.stream_id, h.term_id};
    std::memcpy(at, w, 24);
    at[4] = h.version;
    at[5] = flags;
    std::memcpy(at + 6, &type, 2);
    std::memset(at + 24, 0, 8);
}
}  // namespace

TermAppendResult term_append(std::uint8_t* block, std::size_t len, std::size_t start, const std::uint8_t* data,
                             std::size_t data_len, const std::uint64_t* rec_off, std::size_t n,
                             const TermAppendOptions& options) {
    options.check(len, start);
    const std::uint64_t max_len = options.effective_max_message_length(len), mtu = options.mtu, maxp = mtu - 32;
    TermAppendResult r;
    std::uint64_t tail = start;
    r.stop = SBE_TERM_APPEND_END;
    for (std::size_t i = 0; i < n; ++i) {
        const std::uint64_t lo = rec_off[i], hi = rec_off[i + 1];
        if (hi < lo || hi > data_len) {
            r.stop = SBE_TERM_APPEND_BAD_RECORD;
            break;
        }
        if (tail >= options.limit) {
            r.stop = SBE_TERM_APPEND_LIMIT;
            break;
        }
        const std::uint64_t L = hi - lo;
        if (L > max_len) {
            r.stop = SBE_TERM_APPEND_TOO_LONG;
            break;
        }
        if (tail + term_frames_length(L, options.mtu) > len) {
            if (tail < len) put_header(block + tail, (std::uint32_t)(len - tail), 0xC0, 0, tail, options.header);
            tail = len;
            r.stop = SBE_TERM_APPEND_TRIPPED;
            break;
        }
        std::uint64_t done = 0;
        do {
            const std::uint64_t part = L - done < maxp ? L - done : maxp;
            const std::uint8_t flags = (done == 0 ? 0x80 : 0) | (done + part == L ? 0x40 : 0);
            const std::uint64_t size = (32 + part + 31) & ~31ull;
            put_header(block + tail, (std::uint32_t)(32 + part), flags, 1, tail, options.header);
            if (part) std::memcpy(block + tail + 32, data + lo + done, part);
            std::memset(block + tail + 32 + part, 0, size - 32 - part);
            tail += size;
            done += part;
        } while (done < L);
        r.rec_tail.push_back(tail);
    }
    r.appended = r.rec_tail.size();
    r.next = tail;
    return r;
}

}  // namespace aeron_cluster
