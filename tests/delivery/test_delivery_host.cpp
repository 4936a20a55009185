// DeliveryTracker of the host mirror against a plain std::set / std::map transcription of the
// subscriber's callback (examples/pubsub_reconnect_test.cpp:625-691) and of the publisher's two
// inserts (:455-459, :498-501) over the same sequence.  Prints "delivery host: ok" and exits 0
// when every result agrees.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
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

struct Ref {  // the example's containers and the second half of its callback
    std::set<std::string> received_message_ids, received_client_order_ids, duplicate_client_order_ids, sent_client_order_ids;
    std::map<std::string, int> duplicate_delivery_counts;
    std::map<std::string, std::uint64_t> client_order_send_time;
    std::map<std::string, std::int64_t> client_order_latency;
    std::uint64_t messages_received = 0;

    void publish(const std::string& id, std::uint64_t now) {
        sent_client_order_ids.insert(id);
        client_order_send_time.emplace(id, now);  // the mirror keeps the first send time; no id is sent twice here
    }
    void clear_duplicate_tracking() { duplicate_delivery_counts.clear(); }
    Delivery on_message(const std::string& message_id, const std::string& coid, const std::string& oid, std::uint64_t now) {
        Delivery d;
        d.selected = true;
        d.client_order_id = coid;
        d.order_id = oid;
        if (!message_id.empty()) {
            if (received_message_ids.find(message_id) == received_message_ids.end()) {
                received_message_ids.insert(message_id);
                duplicate_delivery_counts.erase(message_id);
            } else {
                d.already_processed = true;
            }
        }
        if (!d.already_processed) messages_received++;
        if (d.already_processed) {
            d.redeliveries = (std::uint32_t)++duplicate_delivery_counts[message_id];
            if (!coid.empty()) received_client_order_ids.insert(coid);
        } else if (!coid.empty()) {
            if (!received_client_order_ids.insert(coid).second) {
                duplicate_client_order_ids.insert(coid);
                d.duplicate_client_order = true;
            }
        }
        if (!coid.empty()) {
            d.was_sent = sent_client_order_ids.count(coid) != 0;
            auto s = client_order_send_time.find(coid);
            if (s != client_order_send_time.end() && client_order_latency.find(coid) == client_order_latency.end()) {
                d.latency_recorded = true;
                d.latency_ns = (std::int64_t)now - (std::int64_t)s->second;
                client_order_latency[coid] = d.latency_ns;
            }
        }
        return d;
    }
    std::size_t missing() const {
        std::size_t k = 0;
        for (const std::string& s : sent_client_order_ids) k += received_client_order_ids.count(s) == 0;
        return k;
    }
    std::size_t extra() const {
        std::size_t k = 0;
        for (const std::string& s : received_client_order_ids) k += sent_client_order_ids.count(s) == 0;
        return k;
    }
};

void put16(std::string& s, std::size_t v) {
    s.push_back((char)(v & 0xff));
    s.push_back((char)(v >> 8));
}
// a TopicMessage record (blockLength 16, template 1, schema 1): timestamp, sequence, five strings
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
std::string escaped(const std::string& s) {  // the last byte spelled \u00XX: another token, the same string
    char b[8];
    std::snprintf(b, sizeof b, "\\u%04x", (unsigned)(unsigned char)s.back());
    return s.substr(0, s.size() - 1) + b;
}

struct Msg {
    std::string record, message_id, coid, oid;  // what the callback extracts
    bool selected = true;
};
// one order message in one of the payload formats the callback knows
Msg order_message(int fmt, const std::string& mid, const std::string& c, const std::string& o, std::uint64_t ts) {
    Msg m;
    m.message_id = mid;
    std::string p, type = "CREATE_ORDER";
    const std::string qc = "\"" + c + "\"", qo = "\"" + o + "\"";
    switch (fmt) {
        case 0: p = "{\"message\":{\"message\":{\"client_order_id\":" + qc + ",\"order_id\":" + qo + "}},\"uuid\":\"no\"}"; m.coid = c, m.oid = o; break;
        case 1: p = "{\"message\":{\"message\":{\"order_id\":" + qo + ",\"order_details\":{\"client_order_id\":" + qc + "}}}}"; m.coid = c, m.oid = o; break;
        case 2: p = "{\"message\":{\"order_details\":{\"client_order_id\":" + qc + "}}}"; m.coid = c; break;
        case 3: p = "{\"uuid\":" + qo + ",\"message\":{\"message\":{\"client_order_id\":" + qc + "}}}"; m.coid = c, m.oid = o; break;
        case 4: p = "{\"message\":{\"message\":{\"client_order_id\":\"" + escaped(c) + "\",\"order_id\":\"" + escaped(o) + "\"}}}"; m.coid = c, m.oid = o; break;
        case 5: p = "{\"message\":{\"message\":{\"client_order_id\":\"" + escaped(c) + "\",\"order_details\":{\"client_order_id\":\"other\"}}}}"; m.coid = c; break;
        case 6: p = "{\"message\":{\"message\":{\"client_order_id\":17,\"order_id\":" + qo + "}}}"; m.oid = o; break;
        case 7: p = "[" + qc + "]"; break;
        case 8: p = "{\"message\":{\"message\":{\"client_order_id\":" + qc; break;
        case 9: p = ""; break;
        default: type = "HEARTBEAT", p = "{\"message\":{\"text\":" + qc + "}}", m.selected = false; break;
    }
    m.record = topic_message(type, mid, p, ts);
    return m;
}
constexpr int kFormats = 11;

void same(const Delivery& a, const Delivery& b, bool batch_counts) {
    CHECK(a.selected == b.selected);
    if (!b.selected) return;
    CHECK(a.already_processed == b.already_processed);
    if (!batch_counts) CHECK(a.redeliveries == b.redeliveries);
    CHECK(a.client_order_id == b.client_order_id);
    CHECK(a.order_id == b.order_id);
    CHECK(a.duplicate_client_order == b.duplicate_client_order);
    CHECK(a.was_sent == b.was_sent);
    CHECK(a.latency_recorded == b.latency_recorded);
    CHECK(a.latency_ns == b.latency_ns);
}

void totals(const DeliveryTracker& t, const Ref& ref) {
    CHECK(t.messages_received() == ref.messages_received);
    CHECK(t.sent() == ref.sent_client_order_ids.size());
    CHECK(t.received() == ref.received_client_order_ids.size());
    CHECK(t.missing() == ref.missing());
    CHECK(t.extra() == ref.extra());
}
}  // namespace

int main() {
    std::mt19937_64 rng(7);
    // client order ids: uuid-like, some over 40 bytes, families that differ in the last byte
    std::vector<std::string> ids{"c", "d", std::string(40, 'y'), std::string(41, 'y'), std::string(39, 'y') + "z", "ord-1", "ord-2", "ord-"};
    for (int i = 0; i < 400; ++i) {
        char b[64];
        std::snprintf(b, sizeof b, "%08x-%04x-4%03x-%012llx", (unsigned)rng(), (unsigned)(rng() & 0xffff), (unsigned)(rng() & 0xfff),
                      (unsigned long long)(rng() & 0xffffffffffffull));
        ids.push_back(std::string(b) + (i % 9 == 0 ? "-with-a-long-suffix" : ""));
    }
    DeliveryTracker tracker(64, 1);  // grows by rehash from 64 slots
    Ref ref;
    // the publisher sends the first 300 ids in three calls
    for (int part = 0; part < 3; ++part) {
        const std::vector<std::string> some(ids.begin() + 100 * part, ids.begin() + 100 * (part + 1));
        tracker.note_sent(some, 1000 + part);
        for (const std::string& s : some) ref.publish(s, 1000 + part);
    }
    totals(tracker, ref);

    std::vector<Msg> history;
    std::uint64_t serial = 0;
    for (int call = 0; call < 8; ++call) {
        if (call == 5) {
            tracker.clear_duplicate_tracking();
            ref.clear_duplicate_tracking();
        }
        // a batch: new messages in every format, redeliveries of earlier ones, an ack, an undecodable record
        std::vector<Msg> batch;
        const int n = call == 0 ? 1 : 150 + 30 * call;
        for (int j = 0; j < n; ++j) {
            const unsigned r = (unsigned)(rng() % 20);
            if (r < 6 && !history.empty()) {
                batch.push_back(history[rng() % (r < 3 ? std::min<std::size_t>(history.size(), 4) : history.size())]);
            } else if (r == 6) {
                Msg m;
                m.selected = false;
                m.record = j % 2 ? std::string("\x01\x02\x03", 3) : std::string();
                batch.push_back(m);
            } else {
                std::string mid = "msg_" + std::to_string(1760000000000000ull + serial) + "_" + std::to_string(serial);
                ++serial;
                if (r == 7) mid.clear();
                if (r == 8) mid += "_" + std::string(30, 'x');  // over the key limit
                const std::string& c = ids[rng() % ids.size()];
                Msg m = order_message((int)(rng() % kFormats), mid, c, "oid-" + c.substr(0, 20), 50 + j);
                batch.push_back(m);
                if (m.selected && !mid.empty()) history.push_back(m);
            }
        }
        const std::uint64_t now = 5000 + 10 * call;
        if (call % 3 == 2) {  // the single form, record by record
            for (const Msg& m : batch) {
                const ParseResult pr = MessageParser::parse_message(reinterpret_cast<const std::uint8_t*>(m.record.data()), m.record.size());
                const Delivery got = tracker.on_message(pr, now);
                Delivery exp;
                if (m.selected) exp = ref.on_message(m.message_id, m.coid, m.oid, now);
                same(got, exp, false);
            }
        } else {
            std::string data;
            std::vector<std::uint64_t> off{0};
            for (const Msg& m : batch) {
                data += m.record;
                off.push_back(data.size());
            }
            const ParsedBatch pb = MessageParser::decode_batch(reinterpret_cast<const std::uint8_t*>(data.data()), off.data(), batch.size());
            const std::vector<Delivery> got = tracker.on_batch(pb, now);
            CHECK(got.size() == batch.size());
            std::vector<Delivery> exp(batch.size());
            std::map<std::string, std::uint32_t> last;  // the batch form reports an id's count after the whole batch
            for (std::size_t i = 0; i < batch.size(); ++i) {
                if (!batch[i].selected) continue;
                exp[i] = ref.on_message(batch[i].message_id, batch[i].coid, batch[i].oid, now);
                if (exp[i].already_processed) last[batch[i].message_id] = exp[i].redeliveries;
            }
            for (std::size_t i = 0; i < batch.size() && i < got.size(); ++i) {
                same(got[i], exp[i], true);
                if (exp[i].selected && exp[i].already_processed) CHECK(got[i].redeliveries == last[batch[i].message_id]);
                if (exp[i].selected && !exp[i].already_processed) CHECK(got[i].redeliveries == 0);
            }
        }
        totals(tracker, ref);
    }
    CHECK(tracker.rehashes() >= 3);
    CHECK(ref.messages_received > 500 && !ref.duplicate_client_order_ids.empty() && ref.client_order_latency.size() > 100);
    bool five = false;
    for (const auto& kv : ref.duplicate_delivery_counts) five |= kv.second >= 5;
    CHECK(five);
    if (g_bad) {
        std::printf("delivery host: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("delivery host: ok\n");
    return 0;
}
