// FragmentReassembler::on_term_block (sbe_term_scan + sbe_reassemble_fragments on the device)
// against term_walk + on_fragments, over the case file of tests/termscan_lib.py (write_cases; the
// stored expectation is checked against term_walk too).  The blocks of the file are polled one
// after another by one reassembler of each kind, so a message that spans two blocks goes through
// the carry of both.  Prints one line per case ("case k: messages m bytes b pending p next n") and
// "term host: ok" with exit status 0 when every result agrees.
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

int main(int argc, char** argv) {
    if (argc < 2) return 64;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::uint64_t count = 0;
    if (std::fread(&count, 8, 1, f) != 1) return 3;
    FragmentReassembler dev, host;
    int bad = 0;
    for (std::uint64_t k = 0; k < count; ++k) {
        std::uint64_t h[6];
        if (std::fread(h, 8, 6, f) != 6) return 3;
        std::vector<std::uint8_t> block, flags;
        std::vector<std::uint64_t> frag_off;
        std::vector<std::uint32_t> frag_src;
        if (!rd(f, block, h[0]) || !rd(f, frag_off, h[3] + 1) || !rd(f, frag_src, h[3]) || !rd(f, flags, h[3])) return 4;
        const TermFragments t = term_walk(block.data(), block.size(), h[1], h[2]);
        if (t.frag_off != frag_off || t.frag_src != frag_src || t.flags != flags || t.next != h[4] || t.stop != h[5]) {
            std::printf("case %llu: term_walk differs from the stored expectation\n", (unsigned long long)k);
            ++bad;
        }
        std::vector<std::uint8_t> payload(t.frag_off.back());
        for (std::size_t i = 0; i < t.flags.size(); ++i)
            if (t.frag_off[i + 1] > t.frag_off[i])
                std::memcpy(payload.data() + t.frag_off[i], block.data() + t.frag_src[i] + 32, t.frag_off[i + 1] - t.frag_off[i]);
        const EncodedBatch exp = host.on_fragments(payload.data(), t.frag_off.data(), t.flags.data(), t.flags.size());
        std::size_t next = ~(std::size_t)0;
        const EncodedBatch got = dev.on_term_block(block.data(), block.size(), h[1], h[2], &next);
        const std::size_t m = got.offsets.size() ? got.offsets.size() - 1 : 0;
        const bool same = next == t.next && got.offsets.size() == exp.offsets.size() &&
                          std::memcmp(got.offsets.data(), exp.offsets.data(), 8 * got.offsets.size()) == 0 &&
                          got.bytes.size() == exp.bytes.size() &&
                          (got.bytes.size() == 0 || std::memcmp(got.bytes.data(), exp.bytes.data(), got.bytes.size()) == 0) &&
                          dev.pending_bytes() == host.pending_bytes();
        std::printf("case %llu: messages %zu bytes %zu pending %zu next %zu%s\n", (unsigned long long)k, m, got.bytes.size(),
                    dev.pending_bytes(), next, same ? "" : "  DIFFERS from term_walk + on_fragments");
        if (!same) ++bad;
    }
    std::fclose(f);
    if (bad) return 1;
    std::printf("term host: ok\n");
    return 0;
}
