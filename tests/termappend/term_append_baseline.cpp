// The host side of the term_append bench row: the host mirror's one-thread term_append of a batch
// of records (argv[1]: u64 n, rec_off (u64 x n + 1), the record bytes) into a block of argv[2]
// bytes at MTU 1408.  Best of five.  Prints one JSON line.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "aeron_cluster_amd.hpp"

using namespace aeron_cluster;

int main(int argc, char** argv) {
    if (argc < 3) return 64;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::uint64_t n = 0;
    if (std::fread(&n, 8, 1, f) != 1) return 3;
    std::vector<std::uint64_t> off(n + 1);
    if (std::fread(off.data(), 8, n + 1, f) != n + 1) return 3;
    std::vector<std::uint8_t> data(off[n]);
    if (!data.empty() && std::fread(data.data(), 1, data.size(), f) != data.size()) return 3;
    std::fclose(f);
    std::vector<std::uint8_t> block(std::strtoull(argv[2], nullptr, 10));
    TermAppendOptions o;
    o.header = {7, 1001, 3, 0, 1};
    double best = 1e30;
    TermAppendResult r;
    for (int rep = 0; rep < 5; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        r = term_append(block.data(), block.size(), 0, data.data(), data.size(), off.data(), n, o);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        best = ms < best ? ms : best;
    }
    std::printf("{\"block_bytes\": %zu, \"appended\": %zu, \"next\": %llu, \"stop\": %u, \"term_append_ms\": %.4f, \"check\": %u}\n",
                block.size(), r.appended, (unsigned long long)r.next, r.stop, best, (unsigned)block[r.next / 2]);
    return 0;
}
