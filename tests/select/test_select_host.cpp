// The host mirror's use of sbe_order_select, over the edge batch of tests/select_lib.py (argv[1]:
// u64 n, u64 bytes, rec_off [n + 1], the records) followed by order messages in the payload formats
// the subscriber's callback knows:
//   ParsedBatch::order_select() against ParseResult::is_*() and classify_topic of batch.result(i);
//   extract_order_ids(batch) against a loop of extract_order_ids(batch.result(i));
//   DeliveryTracker::on_batch against on_message over the same TopicMessage records with a fresh
//   tracker (the batch form selects no other record).
// Prints "select host: ok" and exits 0 when every result agrees.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "aeron_cluster_amd.hpp"
#include "sbecodec.h"

using namespace aeron_cluster;

namespace {
int g_bad = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c) && g_bad++ < 20) std::printf("line %d: %s (record %zu)\n", __LINE__, #c, g_i); \
    } while (0)
std::size_t g_i = 0;

void put16(std::string& s, std::size_t v) {
    s.push_back((char)(v & 0xff));
    s.push_back((char)(v >> 8));
}
std::string topic_message(const std::string& topic, const std::string& type, const std::string& id, const std::string& payload) {
    std::string s;
    put16(s, 16), put16(s, 1), put16(s, 1), put16(s, 1);
    const std::uint64_t ts = 99, seq = 0;
    s.append(reinterpret_cast<const char*>(&ts), 8);
    s.append(reinterpret_cast<const char*>(&seq), 8);
    for (const std::string& f : {topic, type, id, payload, std::string("{}")}) {
        put16(s, f.size());
        s += f;
    }
    return s;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 64;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::uint64_t h[2];
    if (std::fread(h, 8, 2, f) != 2) return 3;
    std::vector<std::uint64_t> off(h[0] + 1);
    std::string data(h[1], '\0');
    if (std::fread(off.data(), 8, off.size(), f) != off.size() || (h[1] && std::fread(data.data(), 1, h[1], f) != h[1])) return 3;
    std::fclose(f);
    // order messages: selected by type, by payload alone, not at all; ids sent and not sent; redeliveries
    std::vector<std::string> sent;
    for (int k = 0; k < 200; ++k) {
        const std::string c = "coid-" + std::to_string(k % 90), o = "oid-" + std::to_string(k);
        const std::string mid = "msg_" + std::to_string(k % 150);
        std::string p;
        switch (k % 5) {
            case 0: p = "{\"message\":{\"message\":{\"client_order_id\":\"" + c + "\",\"order_id\":\"" + o + "\"}}}"; break;
            case 1: p = "{\"message\":{\"order_details\":{\"client_order_id\":\"" + c + "\"}}}"; break;
            case 2: p = "{\"uuid\":\"" + o + "\",\"message\":{\"message\":{\"client_order_id\":\"" + c + "\"}}}"; break;
            case 3: p = "{\"message\":{\"message\":{\"order_id\":\"" + o + "\"}},\"note\":\"" + c + "\"}"; break;
            default: p = "{\"message\":{\"text\":\"" + c + "\"}}"; break;
        }
        const char* types[4] = {"CREATE_ORDER", "", "HEARTBEAT", "UPDATE_ORDER"};
        data += topic_message(k % 2 ? "orders" : "order_notification_topic", types[(k / 5) % 4], mid, p);
        off.push_back(data.size());
        if (k % 3) sent.push_back(c);
    }
    const std::size_t n = off.size() - 1;
    const ParsedBatch pb = MessageParser::decode_batch(reinterpret_cast<const std::uint8_t*>(data.data()), off.data(), n);

    const MessageKinds kinds = pb.order_select();
    CHECK(kinds.size() == n);
    std::uint64_t n_sel = 0, n_order = 0;
    for (g_i = 0; g_i < n && g_i < kinds.size(); ++g_i) {
        const std::size_t i = g_i;
        const ParseResult r = pb.result(i);
        const unsigned pred = (r.is_session_event() ? SBE_PR_SESSION_EVENT : 0u) | (r.is_topic_message() ? SBE_PR_TOPIC_MESSAGE : 0u) |
                              (r.is_acknowledgment() ? SBE_PR_ACKNOWLEDGMENT : 0u) | (r.is_order_message() ? SBE_PR_ORDER_MESSAGE : 0u);
        CHECK(kinds.pred(i) == pred);
        const bool tm = pb.status(i) == SBE_ST_TM;
        const bool sel = tm && (r.is_order_message() || (r.is_topic_message() && r.message_type == "CREATE_ORDER"));
        CHECK(kinds.selected(i) == sel);
        CHECK(kinds.topic_class(i) == (tm ? classify_topic(pb.view(i, 0)) : TopicClass::Unknown));
        n_sel += sel;
        n_order += r.is_order_message();
    }
    g_i = 0;
    CHECK(kinds.selected_count() == n_sel && kinds.order_count() == n_order);
    CHECK(n_sel > 100 && n_sel + 100 < n);

    const std::vector<OrderIds> ids = extract_order_ids(pb);
    CHECK(ids.size() == n);
    std::size_t with_ids = 0;
    for (g_i = 0; g_i < n && g_i < ids.size(); ++g_i) {
        const OrderIds one = extract_order_ids(pb.result(g_i));
        CHECK(ids[g_i].client_order_id == one.client_order_id && ids[g_i].order_id == one.order_id);
        with_ids += !one.client_order_id.empty();
    }
    g_i = 0;
    CHECK(with_ids > 50);

    DeliveryTracker batch_tracker(64, 1), single_tracker(64, 1);
    batch_tracker.note_sent(sent, 1000);
    single_tracker.note_sent(sent, 1000);
    const std::vector<Delivery> got = batch_tracker.on_batch(pb, 5000);
    CHECK(got.size() == n);
    std::size_t tracked = 0;
    for (g_i = 0; g_i < n && g_i < got.size(); ++g_i) {
        const Delivery& a = got[g_i];
        // The batch form serves TopicMessages only (extract and keys read their views); the
        // one-record form takes any ParseResult, as the example's callback does, so an Ack whose
        // payload holds a needle is selected there and would put its id into the tables.
        if (pb.status(g_i) != SBE_ST_TM) {
            CHECK(!a.selected);
            continue;
        }
        const Delivery exp = single_tracker.on_message(pb.result(g_i), 5000);
        tracked += exp.selected;
        CHECK(a.selected == exp.selected);
        if (!exp.selected) continue;
        CHECK(a.already_processed == exp.already_processed);  // redeliveries: the batch form counts after the whole batch
        CHECK(a.client_order_id == exp.client_order_id && a.order_id == exp.order_id);
        CHECK(a.duplicate_client_order == exp.duplicate_client_order);
        CHECK(a.was_sent == exp.was_sent && a.latency_recorded == exp.latency_recorded && a.latency_ns == exp.latency_ns);
    }
    g_i = 0;
    CHECK(tracked > 300);
    CHECK(batch_tracker.messages_received() == single_tracker.messages_received());
    CHECK(batch_tracker.received() == single_tracker.received() && batch_tracker.missing() == single_tracker.missing());
    if (g_bad) {
        std::printf("select host: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("select host: ok\n");
    return 0;
}
