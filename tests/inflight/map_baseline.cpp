// One thread, std::unordered_map<std::string, std::uint64_t>: the emplace / find / erase sequence of
// ClusterClient::remember_outgoing and on_ack_default (src/cluster_client.cpp:1920-1941) for n
// "pub_<nanos>" uuids and n acks of which about 10 % carry an id nobody sent and 1 % repeat an
// earlier ack's id: the host side of the ack_correlate row of scripts/bench_rows.py.  Prints one
// JSON object with the best of five runs of each phase.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

int main(int argc, char** argv) {
    const std::size_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1000000;
    std::mt19937_64 rng(0x5EED09);
    const std::uint64_t base = 1760000000000000000ull;
    std::vector<std::string> uuids(n), ids(n);
    std::vector<std::uint64_t> ts(n);
    std::uint64_t t = base;
    for (std::size_t i = 0; i < n; ++i) {
        t += 1 + rng() % 2000;
        ts[i] = t;
        uuids[i] = "pub_" + std::to_string(t);
    }
    std::vector<std::size_t> perm(n);
    for (std::size_t i = 0; i < n; ++i) perm[i] = i;
    std::shuffle(perm.begin(), perm.end(), rng);
    for (std::size_t i = 0; i < n; ++i) {
        const unsigned k = (unsigned)(rng() % 100);
        if (k < 10) ids[i] = "pub_" + std::to_string(base - 1 - rng() % 1000000000);
        else if (k == 99 && i) ids[i] = ids[rng() % i];
        else ids[i] = uuids[perm[i]];
    }
    double best_rem = 1e30, best_match = 1e30;
    std::uint64_t matched = 0, sink = 0;
    for (int run = 0; run < 5; ++run) {
        std::unordered_map<std::string, std::uint64_t> inflight;
        const auto t0 = std::chrono::steady_clock::now();
        for (std::size_t i = 0; i < n; ++i) inflight.emplace(uuids[i], ts[i]);
        const auto t1 = std::chrono::steady_clock::now();
        matched = 0;
        const std::uint64_t now = base + 5000000000ull;
        for (std::size_t i = 0; i < n; ++i) {
            auto it = !ids[i].empty() ? inflight.find(ids[i]) : inflight.end();
            if (it != inflight.end()) {
                sink += now - it->second;
                inflight.erase(it);
                ++matched;
            } else {
                sink += now - (base + 5);
            }
        }
        const auto t2 = std::chrono::steady_clock::now();
        best_rem = std::min(best_rem, std::chrono::duration<double, std::milli>(t1 - t0).count());
        best_match = std::min(best_match, std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    std::printf("{\"records\": %zu, \"remember_ms\": %.3f, \"match_ms\": %.3f, \"matched\": %llu, \"runs\": 5, \"sink\": %llu}\n", n,
                best_rem, best_match, (unsigned long long)matched, (unsigned long long)sink);
    return 0;
}
