// The report members of DeliveryTracker (missing_ids, extra_ids, redelivered_ids, latency_report)
// against std::set / std::map / std::sort kept here: the containers of
// examples/pubsub_reconnect_test.cpp and what its printMessageComparison (:130-204) and
// printLatencyReport (:276-353) take from them, over one sequence of batches and single messages
// with ids over 40 bytes in every set and among the latency samples.  Prints "report host: ok"
// and exits 0 when every result agrees.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "aeron_cluster_amd.hpp"

using namespace aeron_cluster;

namespace {
int g_bad = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c) && g_bad++ < 20) std::printf("line %d: %s\n", __LINE__, #c); \
    } while (0)

struct Ref {  // the example's containers, and the part of its callback that fills them
    std::set<std::string> received_message_ids, received_client_order_ids, sent_client_order_ids;
    std::map<std::string, std::uint64_t> duplicate_delivery_counts, client_order_send_time;
    std::map<std::string, std::int64_t> client_order_latency;
    std::map<std::uint64_t, std::int64_t> latency_of_tag;  // this test's: which record a latency came from

    void publish(const std::string& id, std::uint64_t now) {
        sent_client_order_ids.insert(id);
        client_order_send_time.emplace(id, now);
    }
    void on_message(const std::string& message_id, const std::string& coid, std::uint64_t now, std::uint64_t tag) {
        bool already = false;
        if (!message_id.empty()) {
            if (received_message_ids.insert(message_id).second)
                duplicate_delivery_counts.erase(message_id);
            else
                already = true;
        }
        if (already) ++duplicate_delivery_counts[message_id];
        if (coid.empty()) return;
        received_client_order_ids.insert(coid);
        auto s = client_order_send_time.find(coid);
        if (s != client_order_send_time.end() && client_order_latency.find(coid) == client_order_latency.end()) {
            client_order_latency[coid] = (std::int64_t)now - (std::int64_t)s->second;
            latency_of_tag[tag] = client_order_latency[coid];
        }
    }
    static std::vector<std::string> minus(const std::set<std::string>& a, const std::set<std::string>& b) {  // :153-162
        std::vector<std::string> out;
        for (const std::string& s : a)
            if (b.find(s) == b.end()) out.push_back(s);
        return out;  // in std::set order
    }
};

void put16(std::string& s, std::size_t v) {
    s.push_back((char)(v & 0xff));
    s.push_back((char)(v >> 8));
}
std::string topic_message(const std::string& type, const std::string& id, const std::string& payload, std::uint64_t ts) {
    std::string s;
    put16(s, 16), put16(s, 1), put16(s, 1), put16(s, 1);
    const std::uint64_t seq = 0;
    s.append(reinterpret_cast<const char*>(&ts), 8);
    s.append(reinterpret_cast<const char*>(&seq), 8);
    for (const std::string& f : {std::string("order_notification_topic"), type, id, payload, std::string("{}")}) {
        put16(s, f.size());
        s += f;
    }
    return s;
}
struct Msg {
    std::string record, message_id, coid;
    bool selected = true;
};
Msg order_message(int fmt, const std::string& mid, const std::string& c) {
    Msg m;
    m.message_id = mid;
    const std::string qc = "\"" + c + "\"";
    std::string p, type = "CREATE_ORDER";
    switch (fmt) {
        case 0: p = "{\"message\":{\"message\":{\"client_order_id\":" + qc + ",\"order_id\":\"o\"}}}"; m.coid = c; break;
        case 1: p = "{\"message\":{\"message\":{\"order_details\":{\"client_order_id\":" + qc + "}}}}"; m.coid = c; break;
        case 2: p = "{\"message\":{\"order_details\":{\"client_order_id\":" + qc + "}}}"; m.coid = c; break;
        case 3: p = "{\"message\":{\"text\":" + qc + "}}"; break;  // no client order id
        default: type = "HEARTBEAT", p = "{}", m.selected = false; break;
    }
    m.record = topic_message(type, mid, p, 1);
    return m;
}

void same_list(const IdList& got, const std::vector<std::pair<std::string, std::uint64_t>>& all, std::size_t limit, bool values) {
    CHECK(got.total == all.size());
    CHECK(got.first.size() == std::min(limit, all.size()));
    for (std::size_t j = 0; j < got.first.size() && j < all.size(); ++j) {
        CHECK(got.first[j].id == all[j].first);
        if (values) CHECK(got.first[j].value == all[j].second);
    }
}

// printLatencyReport's numbers from the map, in units of `unit`
void same_report(const DeliveryTracker& t, const Ref& ref, const std::vector<double>& pcts, std::uint64_t unit) {
    std::vector<long long> latencies;
    for (const auto& kv : ref.client_order_latency) latencies.push_back(kv.second / (long long)unit);
    std::sort(latencies.begin(), latencies.end());
    auto percentile = [&](double pct) -> long long {  // :318-328
        if (latencies.empty()) return 0;
        double rank = (pct / 100.0) * static_cast<double>(latencies.size());
        size_t idx = rank <= 0.0 ? 0 : static_cast<size_t>(std::ceil(rank)) - 1;
        if (idx >= latencies.size()) idx = latencies.size() - 1;
        return latencies[idx];
    };
    long long sum = 0;
    for (auto v : latencies) sum += v;
    const LatencyReport plain = t.latency_report(pcts, unit, false), rows = t.latency_report(pcts, unit, true);
    for (const LatencyReport* r : {&plain, &rows}) {
        CHECK(r->count == latencies.size());
        CHECK(r->sum == sum);
        CHECK(r->min == (latencies.empty() ? 0 : latencies.front()));
        CHECK(r->max == (latencies.empty() ? 0 : latencies.back()));
        CHECK(r->avg == (latencies.empty() ? 0.0 : static_cast<double>(sum) / static_cast<double>(latencies.size())));
        CHECK(r->percentiles.size() == pcts.size());
        for (std::size_t p = 0; p < pcts.size() && p < r->percentiles.size(); ++p) CHECK(r->percentiles[p] == percentile(pcts[p]));
    }
    CHECK(plain.rows.empty() && rows.rows.size() == latencies.size());
    std::set<std::uint64_t> tags;
    for (std::size_t j = 0; j < rows.rows.size(); ++j) {  // slowest first (:304), each from the record that gave it
        CHECK(rows.rows[j].latency == latencies[latencies.size() - 1 - j]);
        auto it = ref.latency_of_tag.find(rows.rows[j].tag);
        CHECK(it != ref.latency_of_tag.end() && it->second / (long long)unit == rows.rows[j].latency);
        tags.insert(rows.rows[j].tag);
    }
    CHECK(tags.size() == rows.rows.size());
}

void reports(const DeliveryTracker& t, const Ref& ref) {
    std::vector<std::pair<std::string, std::uint64_t>> missing, extra, again;
    for (const std::string& s : Ref::minus(ref.sent_client_order_ids, ref.received_client_order_ids))
        missing.emplace_back(s, ref.client_order_send_time.at(s));
    for (const std::string& s : Ref::minus(ref.received_client_order_ids, ref.sent_client_order_ids)) extra.emplace_back(s, 0);
    for (const auto& kv : ref.duplicate_delivery_counts) again.emplace_back(kv.first, kv.second);
    for (std::size_t limit : {std::size_t(0), std::size_t(1), std::size_t(10), std::size_t(64)}) {
        same_list(t.missing_ids(limit), missing, limit, true);
        same_list(t.extra_ids(limit), extra, limit, false);
        same_list(t.redelivered_ids(limit), again, limit, true);
    }
    CHECK(t.missing() == missing.size() && t.extra() == extra.size());  // the existing counts agree
    const std::vector<double> seven{75.0, 80.0, 90.0, 95.0, 99.0, 99.9, 99.99};
    same_report(t, ref, seven, 1);
    same_report(t, ref, seven, 1000);
    same_report(t, ref, {0.0, 100.0, 50.0}, 7);
    same_report(t, ref, {}, 1000000);
}
}  // namespace

int main() {
    std::mt19937_64 rng(11);
    std::vector<std::string> ids{"c", "d", std::string(40, 'y'), std::string(41, 'y'), std::string(39, 'y') + "z", "ord-1", "ord-"};
    for (int i = 0; i < 400; ++i) {
        char b[64];
        std::snprintf(b, sizeof b, "%08x-%04x-4%03x-%012llx", (unsigned)rng(), (unsigned)(rng() & 0xffff), (unsigned)(rng() & 0xfff),
                      (unsigned long long)(rng() & 0xffffffffffffull));
        ids.push_back(std::string(b) + (i % 7 == 0 ? "-with-a-long-suffix" : ""));  // 56 bytes: the host sets' ids
    }
    DeliveryTracker tracker(64, 1);
    Ref ref;
    reports(tracker, ref);  // nothing tracked yet
    // the first 300 ids are sent; the last hundred of them "later" than they are delivered
    const std::uint64_t sent_at[3] = {1000, 5033, 900000};
    for (int part = 0; part < 3; ++part) {
        const std::vector<std::string> some(ids.begin() + 100 * part, ids.begin() + 100 * (part + 1));
        tracker.note_sent(some, sent_at[part]);
        for (const std::string& s : some) ref.publish(s, sent_at[part]);
    }
    reports(tracker, ref);

    std::vector<Msg> history;
    std::uint64_t serial = 0, calls = 0;
    for (int round = 0; round < 7; ++round) {
        if (round == 5) {
            tracker.clear_duplicate_tracking();
            ref.duplicate_delivery_counts.clear();
        }
        std::vector<Msg> batch;
        const int n = round == 0 ? 1 : 120 + 400 * round;  // the log grows past its first 1024 samples' room
        for (int j = 0; j < n; ++j) {
            const unsigned r = (unsigned)(rng() % 20);
            if (r < 5 && !history.empty()) {
                batch.push_back(history[rng() % (r < 3 ? std::min<std::size_t>(history.size(), 4) : history.size())]);
            } else {
                std::string mid = "msg_" + std::to_string(1760000000000000ull + serial) + "_" + std::to_string(serial);
                ++serial;
                if (r == 7) mid += "_" + std::string(30, 'x');  // over the key limit
                std::size_t pick = rng() % ids.size();
                if (pick % 5 == 2) ++pick;  // every fifth id is never delivered: the sent ones among them stay missing
                Msg m = order_message((int)(rng() % 5), mid, ids[pick]);
                batch.push_back(m);
                if (m.selected) history.push_back(m);
            }
        }
        const std::uint64_t now = 6000 + 1000 * round;
        if (round % 3 == 2) {
            for (const Msg& m : batch) {
                const ParseResult pr = MessageParser::parse_message(reinterpret_cast<const std::uint8_t*>(m.record.data()), m.record.size());
                const Delivery got = tracker.on_message(pr, now);
                CHECK(got.selected == m.selected);
                if (!m.selected) continue;
                ref.on_message(m.message_id, m.coid, now, calls << 32);
                ++calls;
            }
        } else {
            std::string data;
            std::vector<std::uint64_t> off{0};
            for (const Msg& m : batch) {
                data += m.record;
                off.push_back(data.size());
            }
            const ParsedBatch pb = MessageParser::decode_batch(reinterpret_cast<const std::uint8_t*>(data.data()), off.data(), batch.size());
            tracker.on_batch(pb, now);
            for (std::size_t i = 0; i < batch.size(); ++i)
                if (batch[i].selected) ref.on_message(batch[i].message_id, batch[i].coid, now, calls << 32 | i);
            ++calls;
        }
        reports(tracker, ref);
    }
    // the cases this run has to hold
    std::size_t long_missing = 0, long_extra = 0, long_again = 0, long_lat = 0, negative = 0;
    for (const std::string& s : Ref::minus(ref.sent_client_order_ids, ref.received_client_order_ids)) long_missing += s.size() > 40;
    for (const std::string& s : Ref::minus(ref.received_client_order_ids, ref.sent_client_order_ids)) long_extra += s.size() > 40;
    for (const auto& kv : ref.duplicate_delivery_counts) long_again += kv.first.size() > 40;
    for (const auto& kv : ref.client_order_latency) long_lat += kv.first.size() > 40, negative += kv.second < 0;
    CHECK(long_missing && long_extra && long_again && long_lat > 5 && negative > 20);
    // 300 ids are sent and a fifth of them is never delivered: at most 240 latencies
    CHECK(ref.client_order_latency.size() > 200 && ref.client_order_latency.size() <= 240);
    CHECK(ref.duplicate_delivery_counts.size() > 64);
    bool threw = false;
    try {
        tracker.missing_ids(65);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    CHECK(threw);
    if (g_bad) {
        std::printf("report host: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("report host: ok\n");
    return 0;
}
