// CommitManager::serialize_commit_offset and CommitManager::build_commit_offset_fallback (host
// mirror) against cases written by tests/test_commit_fallback_host.py from the composition in
// tests/commitfallback_lib.py.  Runs without a GPU.
//
// File: u64 count, then per case the strings topic, client_id (= message_identifier), message_id
// (u64 length + bytes each), u64 ts, seq, now, uuid clock, the expected text (string), u64 1 + the
// expected record (string) or u64 0 where the reference throws [E100].
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "aeron_cluster_amd.hpp"

using namespace aeron_cluster;

static bool rd64(FILE* f, uint64_t& v) { return std::fread(&v, 8, 1, f) == 1; }
static bool rds(FILE* f, std::string& s) {
    uint64_t n;
    if (!rd64(f, n)) return false;
    s.resize(n);
    return n == 0 || std::fread(&s[0], 1, n, f) == n;
}

int main(int argc, char** argv) {
    if (argc < 2) return 64;
    FILE* f = std::fopen(argv[1], "rb");
    uint64_t count = 0;
    if (!f || !rd64(f, count)) return 2;
    int failures = 0;
    const CommitManager cm;
    for (uint64_t c = 0; c < count; ++c) {
        CommitOffset off;
        std::string text, rec;
        uint64_t now, clock2, has;
        if (!rds(f, off.topic) || !rds(f, off.message_identifier) || !rds(f, off.message_id) ||
            !rd64(f, off.timestamp_nanos) || !rd64(f, off.sequence_number) || !rd64(f, now) || !rd64(f, clock2) ||
            !rds(f, text) || !rd64(f, has) || (has && !rds(f, rec)))
            return 3;
        if (CommitManager::serialize_commit_offset(off) != text) {
            std::printf("case %llu: text differs\n", (unsigned long long)c);
            ++failures;
        }
        int reads = 0;
        bool threw = false;
        std::vector<uint8_t> got;
        try {
            got = cm.build_commit_offset_fallback(off.message_identifier, off, [&] { return reads++ ? clock2 : now; });
        } catch (const std::runtime_error& e) {
            threw = std::string(e.what()) == "buffer too short [E100]";
        }
        const bool ok = has ? (!threw && reads == 2 && std::string(got.begin(), got.end()) == rec) : threw;
        if (!ok) {
            std::printf("case %llu: record differs (threw %d, reads %d, %zu bytes, expected %s)\n", (unsigned long long)c,
                        (int)threw, reads, got.size(), has ? std::to_string(rec.size()).c_str() : "E100");
            ++failures;
        }
    }
    std::fclose(f);
    // the default clock: two system readings, the second not before the first
    const std::vector<uint8_t> r = cm.build_commit_offset_fallback("c", CommitOffset{"t", "c", "m", 1, 2});
    uint64_t ts = 0;
    for (int b = 0; b < 8; ++b) ts |= (uint64_t)r[8 + b] << (8 * b);
    if (r.size() < 63 || ts < 1500000000000000000ull) ++failures;
    if (failures) {
        std::printf("fallback host cpu test: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("fallback host cpu test: ok (%llu cases)\n", (unsigned long long)count);
    return 0;
}
