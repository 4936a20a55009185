// One thread, the reports of examples/pubsub_reconnect_test.cpp over its own containers, in its own
// code shape: the two std::set differences of printMessageComparison (:147-163) with the first ten
// of each (:166-191), and printLatencyReport's std::sort of the rows (:304) and of the latencies
// (:317), its sum and its seven percentiles (:318-348).  n sent client order ids ("cid_<17 digits>",
// the delivery_report row's shape), about 1 % of them never received, about 1 % of the received
// ids never sent, one latency per received sent id.  The host side of the delivery_report row of
// scripts/bench_rows.py.  Prints one JSON object with the best of five runs.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

int main(int argc, char** argv) {
    const std::size_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1000000;
    std::mt19937_64 rng(0x5EED0FA);
    std::set<std::string> sent_client_order_ids, received_client_order_ids;
    std::map<std::string, long long> client_order_latency_ms;
    char b[64];
    for (std::size_t i = 0; i < n; ++i) {
        std::snprintf(b, sizeof b, "cid_%017llu", (unsigned long long)(rng() % 100000000000000000ull));
        sent_client_order_ids.insert(b);
        if (rng() % 100 != 0) {
            received_client_order_ids.insert(b);
            client_order_latency_ms[b] = (long long)(rng() % 2000000) - 1000;
        }
        if (rng() % 100 == 0) {
            std::snprintf(b, sizeof b, "xid_%017llu", (unsigned long long)(rng() % 100000000000000000ull));
            received_client_order_ids.insert(b);
        }
    }
    double best = 1e30, best_sets = 1e30, best_lat = 1e30;
    std::size_t missing_n = 0, extra_n = 0, count = 0;
    long long sink = 0, pcts[7] = {0};
    for (int run = 0; run < 5; ++run) {
        const auto t0 = std::chrono::steady_clock::now();
        std::set<std::string> missing_client_orders, extra_client_orders;
        for (const auto& cid : sent_client_order_ids)
            if (received_client_order_ids.find(cid) == received_client_order_ids.end()) missing_client_orders.insert(cid);
        for (const auto& cid : received_client_order_ids)
            if (sent_client_order_ids.find(cid) == sent_client_order_ids.end()) extra_client_orders.insert(cid);
        int shown = 0;
        for (const auto& id : missing_client_orders) {
            sink += id.size();
            if (++shown >= 10) break;
        }
        shown = 0;
        for (const auto& id : extra_client_orders) {
            sink += id.size();
            if (++shown >= 10) break;
        }
        const auto t1 = std::chrono::steady_clock::now();
        struct Row {
            long long latency_ms;
            std::string client_order_id;
        };
        std::vector<Row> rows;
        std::vector<long long> latencies_ms;
        rows.reserve(client_order_latency_ms.size());
        latencies_ms.reserve(client_order_latency_ms.size());
        for (const auto& kv : client_order_latency_ms) {
            rows.push_back(Row{kv.second, kv.first});
            latencies_ms.push_back(kv.second);
        }
        std::sort(rows.begin(), rows.end(), [](const Row& x, const Row& y) { return x.latency_ms > y.latency_ms; });
        std::sort(latencies_ms.begin(), latencies_ms.end());
        auto percentile = [&](double pct) -> long long {
            if (latencies_ms.empty()) return 0;
            double rank = (pct / 100.0) * static_cast<double>(latencies_ms.size());
            size_t idx = rank <= 0.0 ? 0 : static_cast<size_t>(std::ceil(rank)) - 1;
            if (idx >= latencies_ms.size()) idx = latencies_ms.size() - 1;
            return latencies_ms[idx];
        };
        long long sum = 0;
        for (auto v : latencies_ms) sum += v;
        const double pv[7] = {75.0, 80.0, 90.0, 95.0, 99.0, 99.9, 99.99};
        for (int p = 0; p < 7; ++p) pcts[p] = percentile(pv[p]);
        sink += sum + (rows.empty() ? 0 : rows.front().latency_ms);
        const auto t2 = std::chrono::steady_clock::now();
        missing_n = missing_client_orders.size();
        extra_n = extra_client_orders.size();
        count = latencies_ms.size();
        best_sets = std::min(best_sets, std::chrono::duration<double, std::milli>(t1 - t0).count());
        best_lat = std::min(best_lat, std::chrono::duration<double, std::milli>(t2 - t1).count());
        best = std::min(best, std::chrono::duration<double, std::milli>(t2 - t0).count());
    }
    std::printf("{\"sent\": %zu, \"missing\": %zu, \"extra\": %zu, \"latencies\": %zu, \"report_ms\": %.3f, \"set_differences_ms\": %.3f, "
                "\"latency_report_ms\": %.3f, \"p99_9\": %lld, \"runs\": 5, \"sink\": %lld}\n",
                n, missing_n, extra_n, count, best, best_sets, best_lat, pcts[5], sink);
    return 0;
}
