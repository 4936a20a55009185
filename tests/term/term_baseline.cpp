// The host side of the term_scan bench row: the host mirror's one-thread term_walk over a block
// (argv[1]: the raw block bytes as a file), alone and followed by the memcpy of every payload into
// one compact buffer (what a host poll hands on before reassembly).  Best of five.  Prints one JSON
// line.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "aeron_cluster_amd.hpp"

using namespace aeron_cluster;

int main(int argc, char** argv) {
    if (argc < 2) return 64;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const long len = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<std::uint8_t> block((std::size_t)len);
    if (len && std::fread(block.data(), 1, block.size(), f) != block.size()) return 3;
    std::fclose(f);
    std::vector<std::uint8_t> out(block.size() + 1);
    double walk = 1e30, both = 1e30;
    std::size_t frags = 0, bytes = 0;
    for (int rep = 0; rep < 5; ++rep) {
        auto t0 = std::chrono::steady_clock::now();
        TermFragments t = term_walk(block.data(), block.size(), 0, ~(std::size_t)0);
        const double w = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        walk = w < walk ? w : walk;
        t0 = std::chrono::steady_clock::now();
        t = term_walk(block.data(), block.size(), 0, ~(std::size_t)0);
        for (std::size_t i = 0; i < t.flags.size(); ++i)
            std::memcpy(out.data() + t.frag_off[i], block.data() + t.frag_src[i] + 32, t.frag_off[i + 1] - t.frag_off[i]);
        const double b = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        both = b < both ? b : both;
        frags = t.flags.size();
        bytes = t.frag_off.back();
    }
    std::printf("{\"block_bytes\": %ld, \"fragments\": %zu, \"payload_bytes\": %zu, \"term_walk_ms\": %.4f, "
                "\"term_walk_memcpy_ms\": %.4f, \"check\": %u}\n", len, frags, bytes, walk, both, (unsigned)out[bytes / 2]);
    return 0;
}
