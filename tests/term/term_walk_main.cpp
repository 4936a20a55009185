// TEST ONLY: a stand-alone host program over the host mirror's term_walk (host/term_walk.cpp), built
// plain and with -fsanitize=address,undefined.  It reads the case files tests/termscan_lib.py
// writes (write_cases) and runs term_walk over every block, each in a heap block of exactly its
// size (so a read one byte outside it is reported), and compares every table with the expectation
// stored in the file (the Python restatement's).  Exit status 0: every case matched.
//
// File: u64 count, then per case u64 {block bytes, start, limit, fragments, next, stop}, the block,
// frag_off (u64 x fragments + 1), frag_src (u32 x fragments), flags (u8 x fragments).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "aeron_cluster_amd.hpp"

template <class T>
static bool rd(FILE* f, std::vector<T>& v, std::uint64_t count) {
    v.resize(count);
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

static int run(const char* path, std::uint64_t& cases) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    std::uint64_t count = 0;
    if (std::fread(&count, 8, 1, f) != 1) return 3;
    for (std::uint64_t k = 0; k < count; ++k, ++cases) {
        std::uint64_t h[6];
        if (std::fread(h, 8, 6, f) != 6) return 3;
        std::vector<std::uint8_t> block, flags;
        std::vector<std::uint64_t> frag_off;
        std::vector<std::uint32_t> frag_src;
        if (!rd(f, block, h[0]) || !rd(f, frag_off, h[3] + 1) || !rd(f, frag_src, h[3]) || !rd(f, flags, h[3])) return 4;
        const aeron_cluster::TermFragments t = aeron_cluster::term_walk(block.data(), block.size(), h[1], h[2]);
        if (t.frag_off != frag_off || t.frag_src != frag_src || t.flags != flags || t.next != h[4] || t.stop != h[5]) {
            std::fprintf(stderr, "case %llu: got %zu fragments, next %llu, stop %u; expected %llu, %llu, %llu\n",
                         (unsigned long long)k, t.flags.size(), (unsigned long long)t.next, t.stop,
                         (unsigned long long)h[3], (unsigned long long)h[4], (unsigned long long)h[5]);
            return 5;
        }
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 64;
    std::uint64_t cases = 0;
    for (int i = 1; i < argc; ++i) {
        const int rc = run(argv[i], cases);
        if (rc) {
            std::fprintf(stderr, "%s: mismatch or bad file (%d)\n", argv[i], rc);
            return 1;
        }
    }
    std::printf("term walk: %llu cases ok\n", (unsigned long long)cases);
    return 0;
}
