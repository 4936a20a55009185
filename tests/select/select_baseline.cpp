// The host loop sbe_order_select replaces, timed for the order_select bench row: for every
// TopicMessage of a decoded batch build the ParseResult (ParsedBatch::result_into) and run the
// subscriber's test on it (examples/pubsub_reconnect_test.cpp:578-579), as extract_order_ids and
// DeliveryTracker::on_batch did to fill their mask.  argv: n, case (0: CREATE_ORDER types, flat
// payload; 1: empty type, nested payload), threads.  Prints one JSON line.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "aeron_cluster_amd.hpp"

using namespace aeron_cluster;

static void put16(std::string& s, std::size_t v) {
    s.push_back((char)(v & 0xff));
    s.push_back((char)(v >> 8));
}

int main(int argc, char** argv) {
    const std::size_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1000000;
    const int which = argc > 2 ? std::atoi(argv[2]) : 0;
    const unsigned threads = argc > 3 ? (unsigned)std::atoi(argv[3]) : 1;
    // a fixed-256 Order: topic 6, type 12, uuid 29, payload 143, headers 32
    std::string payload = which ? "{\"uuid\":\"cid_0123456789abcdefg\",\"message\":{\"message\":{\"order_details\":"
                                  "{\"client_order_id\":\"cid_0123456789abcdefg\"}}}}"
                                : "{\"side\":\"BUY\",\"symbol\":\"BTC-USD\",\"qty\":\"000001234\",\"price\":\"00000067890.12\","
                                  "\"client_order_id\":\"cid_00000000000000017\",\"type\":\"LIMIT\",\"tif\":\"GTC\"}";
    payload.resize(143, ' ');
    const std::string type = which ? std::string() : std::string("CREATE_ORDER");
    std::string rec;
    put16(rec, 16), put16(rec, 1), put16(rec, 1), put16(rec, 1);
    rec.append(16, '\0');
    for (const std::string& f : {std::string("orders"), type, std::string("msg_1760000000000000000_00017") + std::string(12 - type.size(), 'x'),
                                 payload, std::string("{\"messageType\":\"CREATE_ORDER\"}  ")}) {
        put16(rec, f.size());
        rec += f;
    }
    std::string data;
    data.reserve(rec.size() * n);
    std::vector<std::uint64_t> off(n + 1, 0);
    for (std::size_t i = 0; i < n; ++i) {
        data += rec;
        off[i + 1] = data.size();
    }
    const ParsedBatch pb = MessageParser::decode_batch(reinterpret_cast<const std::uint8_t*>(data.data()), off.data(), n);
    std::vector<std::uint8_t> select(n, 0);
    auto loop = [&](std::size_t x, std::size_t y) {
        ParseResult r;
        for (std::size_t i = x; i < y; ++i) {
            if (pb.status(i) != 0) continue;
            pb.result_into(i, r);
            select[i] = (r.is_order_message() || (r.is_topic_message() && r.message_type == "CREATE_ORDER")) ? 1 : 0;
        }
    };
    double best = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        if (threads <= 1) {
            loop(0, n);
        } else {
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < threads; ++t) pool.emplace_back(loop, n * t / threads, n * (t + 1) / threads);
            for (std::thread& th : pool) th.join();
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        best = ms < best ? ms : best;
    }
    std::size_t sel = 0;
    for (std::uint8_t s : select) sel += s;
    std::printf("{\"n\": %zu, \"case\": %d, \"threads\": %u, \"record_bytes\": %zu, \"mask_loop_ms\": %.3f, \"selected\": %zu}\n", n, which,
                threads, rec.size(), best, sel);
    return 0;
}
