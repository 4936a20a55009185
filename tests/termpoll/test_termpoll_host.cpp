// FragmentReassembler::poll_term_block (the one call sbe_term_poll) beside on_term_block
// (sbe_term_scan + sbe_reassemble_fragments) and term_walk + on_fragments, over the case file of
// tests/termscan_lib.py (write_cases).  The blocks of the file are polled one after another by one
// reassembler of each kind, so a message that spans two blocks goes through the carry of all
// three.  After every block the three must agree on the returned bytes and offsets, on *next, and
// on the pending accumulator (its size here, its bytes through the next call; a last block of one
// END frame flushes it at the end).  Prints one line per case ("case k: messages m bytes b pending p
// next n") and "term poll host: ok" with exit status 0 when every result agrees.
//
// With --bench: both calls on one 16 MiB block of framed records (wall clock, best of five each,
// after one call of each to warm up), for the row of DESIGN.md.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "aeron_cluster_amd.hpp"
#include "sbecodec.h"

using namespace aeron_cluster;

template <class T>
static bool rd(FILE* f, std::vector<T>& v, std::uint64_t count) {
    v.resize(count);
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

static bool same_batch(const EncodedBatch& a, const EncodedBatch& b) {
    return a.offsets.size() == b.offsets.size() &&
           std::memcmp(a.offsets.data(), b.offsets.data(), 8 * a.offsets.size()) == 0 && a.bytes.size() == b.bytes.size() &&
           (a.bytes.size() == 0 || std::memcmp(a.bytes.data(), b.bytes.data(), a.bytes.size()) == 0);
}

static void frame(std::vector<std::uint8_t>& b, std::uint32_t payload, std::uint8_t flags, std::uint16_t type, std::uint32_t& seed) {
    const std::size_t at = b.size(), n = 32 + payload;
    b.resize(at + ((n + 31) & ~(std::size_t)31), 0);
    const std::int32_t L = (std::int32_t)n;
    std::memcpy(&b[at], &L, 4);
    b[at + 5] = flags;
    std::memcpy(&b[at + 6], &type, 2);
    for (std::uint32_t i = 0; i < payload; ++i) b[at + 32 + i] = (std::uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
}

static int bench() {
    const std::size_t total = 16u << 20;
    std::vector<std::uint8_t> b;
    std::uint32_t seed = 7;
    b.reserve(total);
    while (b.size() + 8 * 1408 < total) {  // 280-byte records, every sixteenth one 4000 bytes in three frames
        if (((seed = seed * 1664525u + 1013904223u) >> 28) == 0) {
            frame(b, 1376, 0x80, 1, seed);
            frame(b, 1376, 0x00, 1, seed);
            frame(b, 1248, 0x40, 1, seed);
        } else {
            frame(b, 280, 0xC0, 1, seed);
        }
    }
    frame(b, (std::uint32_t)(total - b.size() - 32), 0, 0, seed);  // the tail: a padding frame
    double best[2] = {1e30, 1e30};
    std::size_t msgs[2] = {0, 0};
    for (int rep = 0; rep < 6; ++rep)
        for (int which = 0; which < 2; ++which) {
            FragmentReassembler r;
            std::size_t next = 0;
            const auto t0 = std::chrono::steady_clock::now();
            const EncodedBatch e = which ? r.poll_term_block(b.data(), b.size(), 0, ~(std::size_t)0, &next)
                                         : r.on_term_block(b.data(), b.size(), 0, ~(std::size_t)0, &next);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (next != b.size()) return 1;
            msgs[which] = e.offsets.size() - 1;
            if (rep && ms < best[which]) best[which] = ms;  // the first call of each warms up
        }
    if (msgs[0] != msgs[1]) return 1;
    std::printf("term poll host bench: block %zu bytes, %zu messages, on_term_block %.3f ms, poll_term_block %.3f ms "
                "(wall clock, best of five)\n", b.size(), msgs[0], best[0], best[1]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 64;
    if (std::strcmp(argv[1], "--bench") == 0) return bench();
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::uint64_t count = 0;
    if (std::fread(&count, 8, 1, f) != 1) return 3;
    FragmentReassembler poll, dev, host;
    int bad = 0;
    for (std::uint64_t k = 0; k <= count; ++k) {
        std::uint64_t h[6] = {64, 0, ~0ull >> 2, 0, 0, 0};
        std::vector<std::uint8_t> block, flags;
        std::vector<std::uint64_t> frag_off;
        std::vector<std::uint32_t> frag_src;
        if (k < count) {
            if (std::fread(h, 8, 6, f) != 6) return 3;
            if (!rd(f, block, h[0]) || !rd(f, frag_off, h[3] + 1) || !rd(f, frag_src, h[3]) || !rd(f, flags, h[3])) return 4;
        } else {  // behind the file's cases: one END frame, which delivers whatever is still pending
            std::uint32_t seed = 1;
            frame(block, 5, 0x40, 1, seed);
        }
        const TermFragments t = term_walk(block.data(), block.size(), h[1], h[2]);
        if (k < count && (t.frag_off != frag_off || t.frag_src != frag_src || t.flags != flags || t.next != h[4] || t.stop != h[5])) {
            std::printf("case %llu: term_walk differs from the stored expectation\n", (unsigned long long)k);
            ++bad;
        }
        std::vector<std::uint8_t> payload(t.frag_off.back());
        for (std::size_t i = 0; i < t.flags.size(); ++i)
            if (t.frag_off[i + 1] > t.frag_off[i])
                std::memcpy(payload.data() + t.frag_off[i], block.data() + t.frag_src[i] + 32, t.frag_off[i + 1] - t.frag_off[i]);
        const EncodedBatch exp = host.on_fragments(payload.data(), t.frag_off.data(), t.flags.data(), t.flags.size());
        std::size_t next_dev = ~(std::size_t)0, next_poll = ~(std::size_t)0;
        const EncodedBatch old = dev.on_term_block(block.data(), block.size(), h[1], h[2], &next_dev);
        const EncodedBatch got = poll.poll_term_block(block.data(), block.size(), h[1], h[2], &next_poll);
        const std::size_t m = got.offsets.size() ? got.offsets.size() - 1 : 0;
        const bool same = next_poll == t.next && next_poll == next_dev && same_batch(got, exp) && same_batch(got, old) &&
                          poll.pending_bytes() == host.pending_bytes() && poll.pending_bytes() == dev.pending_bytes();
        std::printf("case %llu: messages %zu bytes %zu pending %zu next %zu%s\n", (unsigned long long)k, m, got.bytes.size(),
                    poll.pending_bytes(), next_poll, same ? "" : "  DIFFERS from on_term_block or term_walk + on_fragments");
        if (!same) ++bad;
    }
    std::fclose(f);
    if (bad) return 1;
    std::printf("term poll host: ok\n");
    return 0;
}
