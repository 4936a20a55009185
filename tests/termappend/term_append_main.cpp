// TEST ONLY: a stand-alone host program over the host mirror's term_append (host/term_append.cpp),
// built plain and with -fsanitize=address,undefined.  It reads the case files tests/termappend_lib.py
// writes (write_cases) and runs term_append over every case, the block and the input each in a heap
// block of exactly their size (so a byte read or written outside either is reported), and compares
// the block, the counts and the tails with the expectation stored in the file (the Python
// restatement's).  Exit status 0: every case matched.
//
// File: u64 count, then per case u64 {block bytes, start, limit, mtu, max_message_length, in bytes,
// n, appended, next, payload, stop}, i32 {session, stream, term, base, version}, the input bytes,
// rec_off (u64 x n + 1), rec_tail (u64 x appended), the expected block (the call runs on a block
// filled with 0xA5).
#include <cstdint>
#include <cstdio>
#include <cstring>
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
        std::uint64_t h[11];
        std::int32_t id[5];
        if (std::fread(h, 8, 11, f) != 11 || std::fread(id, 4, 5, f) != 5) return 3;
        std::vector<std::uint8_t> in, expect;
        std::vector<std::uint64_t> rec_off, rec_tail;
        if (!rd(f, in, h[5]) || !rd(f, rec_off, h[6] + 1) || !rd(f, rec_tail, h[7]) || !rd(f, expect, h[0])) return 4;
        aeron_cluster::TermAppendOptions o;
        o.mtu = (std::uint32_t)h[3];
        o.limit = h[2];
        o.max_message_length = h[4];
        o.header = {id[0], id[1], id[2], id[3], (std::uint8_t)id[4]};
        std::vector<std::uint8_t> block(h[0], 0xA5);
        const aeron_cluster::TermAppendResult r =
            aeron_cluster::term_append(block.data(), block.size(), h[1], in.data(), in.size(), rec_off.data(), h[6], o);
        const std::uint64_t payload = rec_off[r.appended] - rec_off[0];
        if (block != expect || r.appended != h[7] || r.next != h[8] || payload != h[9] || r.stop != h[10] || r.rec_tail != rec_tail) {
            std::fprintf(stderr, "case %llu: got appended %zu, next %llu, stop %u; expected %llu, %llu, %llu%s\n",
                         (unsigned long long)k, r.appended, (unsigned long long)r.next, r.stop, (unsigned long long)h[7],
                         (unsigned long long)h[8], (unsigned long long)h[10], block != expect ? "; the block differs" : "");
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
    std::printf("term append: %llu cases ok\n", (unsigned long long)cases);
    return 0;
}
