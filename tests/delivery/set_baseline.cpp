// One thread, the std::set / std::map containers of examples/pubsub_reconnect_test.cpp and the second
// half of its subscriber callback (:625-691) for n deliveries of which about 10 % repeat an earlier
// message, against n sent client order ids: the host side of the delivery_track row of
// scripts/bench_rows.py.  The ids have the row's shapes ("msg_<19 digits>_<5 digits>",
// "cid_<17 digits>").  Prints one JSON object with the best of five runs.
#include <algorithm>
#include <chrono>
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
    std::mt19937_64 rng(0x5EED0F9);
    std::vector<std::string> mid(n), cid(n), sent(n);
    char b[64];
    for (std::size_t i = 0; i < n; ++i) {
        std::snprintf(b, sizeof b, "cid_%017llu", (unsigned long long)(rng() % 100000000000000000ull));
        sent[i] = b;
    }
    for (std::size_t i = 0; i < n; ++i) {
        if (i && rng() % 10 == 0) {  // a redelivery
            const std::size_t j = rng() % i;
            mid[i] = mid[j];
            cid[i] = cid[j];
        } else {
            std::snprintf(b, sizeof b, "msg_%019llu_%05u", 1760000000000000000ull + i, (unsigned)(rng() % 100000));
            mid[i] = b;
            cid[i] = sent[i];
        }
    }
    double best = 1e30, best_sent = 1e30;
    std::uint64_t received = 0, again = 0, recorded = 0, sink = 0;
    for (int run = 0; run < 5; ++run) {
        std::set<std::string> received_message_ids, received_client_order_ids, duplicate_client_order_ids, sent_client_order_ids;
        std::map<std::string, int> duplicate_delivery_counts;
        std::map<std::string, std::uint64_t> client_order_send_time;
        std::map<std::string, std::int64_t> client_order_latency;
        const auto t0 = std::chrono::steady_clock::now();
        for (std::size_t i = 0; i < n; ++i) {
            sent_client_order_ids.insert(sent[i]);
            client_order_send_time[sent[i]] = 1000 + i;
        }
        const auto t1 = std::chrono::steady_clock::now();
        received = again = recorded = 0;
        const std::uint64_t now = 5000000000ull;
        for (std::size_t i = 0; i < n; ++i) {
            const std::string& m = mid[i];
            const std::string& c = cid[i];
            bool already = false;
            if (!m.empty()) {
                if (received_message_ids.find(m) == received_message_ids.end()) {
                    received_message_ids.insert(m);
                    duplicate_delivery_counts.erase(m);
                } else {
                    already = true;
                }
            }
            if (!already) ++received;
            if (already) {
                sink += ++duplicate_delivery_counts[m];
                ++again;
                if (!c.empty()) received_client_order_ids.insert(c);
            } else if (!c.empty()) {
                if (!received_client_order_ids.insert(c).second) duplicate_client_order_ids.insert(c);
            }
            if (!c.empty()) {
                sink += sent_client_order_ids.find(c) != sent_client_order_ids.end();
                auto s = client_order_send_time.find(c);
                if (s != client_order_send_time.end() && client_order_latency.find(c) == client_order_latency.end()) {
                    client_order_latency[c] = (std::int64_t)(now - s->second);
                    ++recorded;
                }
            }
        }
        const auto t2 = std::chrono::steady_clock::now();
        best_sent = std::min(best_sent, std::chrono::duration<double, std::milli>(t1 - t0).count());
        best = std::min(best, std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    std::printf("{\"records\": %zu, \"note_sent_ms\": %.3f, \"callback_ms\": %.3f, \"messages_received\": %llu, \"redeliveries\": %llu, "
                "\"latencies\": %llu, \"runs\": 5, \"sink\": %llu}\n",
                n, best_sent, best, (unsigned long long)received, (unsigned long long)again, (unsigned long long)recorded,
                (unsigned long long)sink);
    return 0;
}
