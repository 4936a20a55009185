// AutoCommitter::commit_and_send_batch (host mirror): a batch whose commit decisions and topic
// texts are written out by hand is committed and sent; the CommitManager must end up as
// commit_record_by_record leaves it, and the sink must receive exactly the frames composed here by
// hand from those expectations, in record order, with and without a callback mask, with last_only
// and without the session frame.  Records whose topic the device table does not hold but
// topic_to_id knows (plain and escaped spellings) appear at their place; topics with id 0 land in
// `unsent`.  Needs a GPU (run by tests/test_gpu_commit_send_host.py).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "aeron_cluster_amd.hpp"
#include "sbecodec.h"

using namespace aeron_cluster;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

typedef std::vector<uint8_t> Bytes;

static void put_le(Bytes& b, uint64_t v, int bytes) {
    for (int k = 0; k < bytes; ++k) b.push_back((uint8_t)(v >> (8 * k)));
}
static void put_str(Bytes& b, const std::string& s) {
    put_le(b, s.size(), 2);
    b.insert(b.end(), s.begin(), s.end());
}
static Bytes tm_wire(const std::string& type, const std::string& id, const std::string& payload,
                     const std::string& headers, uint64_t ts) {
    Bytes b = {16, 0, 1, 0, 1, 0, 1, 0};
    put_le(b, ts, 8);
    put_le(b, 0, 8);
    put_str(b, "orders");
    put_str(b, type);
    put_str(b, id);
    put_str(b, payload);
    put_str(b, headers);
    return b;
}
// send_commit_offset's frame (src/cluster_client.cpp:1264-1278, src/commit_manager.cpp:107-132)
static Bytes frame(const CommitSendOptions& o, uint32_t tid, uint64_t seq, const std::string& id,
                   const std::string& ident) {
    Bytes b;
    if (o.session_frame) {
        for (uint16_t v : {24, 1, 111, 8}) put_le(b, v, 2);
        put_le(b, (uint64_t)o.leadership_term_id, 8);
        put_le(b, (uint64_t)o.cluster_session_id, 8);
        put_le(b, 0, 8);
    }
    for (uint16_t v : {12, 301, 1, 1}) put_le(b, v, 2);
    put_le(b, tid, 4);
    put_le(b, seq, 8);
    put_str(b, id);
    put_str(b, ident);
    return b;
}

struct Case {
    std::string type, id, payload, headers;
    bool commits;
    std::string topic;  // the text extract_topic_from_message returns, when it commits
    uint64_t seq;
};

static bool same(const CommitManager& a, const CommitManager& b) {
    const auto x = a.get_all_commits(), y = b.get_all_commits();
    if (x.size() != y.size()) return false;
    for (const auto& kv : x) {
        auto it = y.find(kv.first);
        if (it == y.end()) return false;
        const CommitOffset &p = kv.second, &q = it->second;
        if (p.topic != q.topic || p.message_identifier != q.message_identifier || p.message_id != q.message_id ||
            p.timestamp_nanos != q.timestamp_nanos || p.sequence_number != q.sequence_number)
            return false;
    }
    return true;
}

int main() {
    const std::string P = "{\"x\":1}";
    const std::vector<Case> base = {
        {"CREATE_ORDER", "m1", P, "{}", true, "orders", 0},                                           // the fallback entry, id 3
        {"X", "m2", "{\"_sequence_number\":41}", "{\"topic\":\"order_notification_topic\"}", true, "order_notification_topic", 41},
        {"X", "m3", P, "{\"topic\":\"alpha\"}", true, "alpha", 0},                                    // a table entry with id 0
        {"X", "m4", "{\"topic\":\"order_request_topic\",\"_sequence_number\":\"7\"}", "", true, "order_request_topic", 7},  // not in the table, id 1
        {"X", "m5", P, "{\"topic\":\"order_\\u0072equest_topic\"}", true, "order_request_topic", 0},  // the same, escaped
        {"X", "m6", P, "{\"topic\":\"order_n\\u006ftification_topic\"}", true, "order_notification_topic", 0},  // an entry, escaped
        {"X", "m7", P, "{\"topic\":\"gamma\"}", true, "gamma", 0},                                    // unknown everywhere
        {"X", "m8", P, "{\"topic\":12}", true, "12", 0},                                              // Value::asString, id 0
        {"X", "m9", P, "{\"topic\":\"order_status_request_topic\"}", true, "order_status_request_topic", 0},  // id 4
        {"SUBSCRIBE", "m10", P, "{}", false, "", 0},
        {"X", "ack_11", P, "{}", false, "", 0},
        {"X", "", P, "{}", false, "", 0},
        {"X", "m13", "", "{}", false, "", 0},
    };
    std::vector<Case> cases;
    for (int round = 0; round < 11; ++round)
        for (size_t j = 0; j < base.size(); ++j) {
            Case c = base[(j * 5 + round * 7) % base.size()];
            if (!c.id.empty() && c.id.compare(0, 4, "ack_") != 0) c.id += "_r" + std::to_string(round);
            cases.push_back(c);
        }
    cases.insert(cases.begin() + 40, Case{"X", std::string(65535, 'L'), P, "{}", true, "orders", 0});  // E109
    cases.insert(cases.begin() + 90, Case{"X", std::string(65534, 'M'), P, "{}", true, "orders", 0});  // the longest id
    Bytes data;
    std::vector<uint64_t> off = {0};
    for (size_t i = 0; i < cases.size(); ++i) {
        const Bytes r = tm_wire(cases[i].type, cases[i].id, cases[i].payload, cases[i].headers, 1000 + i);
        data.insert(data.end(), r.begin(), r.end());
        off.push_back(data.size());
    }
    const size_t n = cases.size();

    AutoCommitter ac("cli", "orders");
    ac.set_message_identifier("order_notification_topic", "id-notif");
    ac.set_message_identifier("alpha", "id-alpha");
    ac.set_message_identifier("never", "");
    const std::vector<std::string> table = {"orders", "alpha", "never", "order_notification_topic"};

    const ParsedBatch batch = MessageParser::decode_batch(data.data(), off.data(), n);
    const CommitPlan plan = ac.classify(batch);
    CHECK(plan.table == table);
    for (size_t i = 0; i < n; ++i) {
        CHECK((plan.cm[i] == SBE_CM_COMMIT) == cases[i].commits);
        if (cases[i].commits) CHECK(ac.topic(batch, plan, i) == cases[i].topic && batch.sequence_number(i) == cases[i].seq);
    }

    for (int mode = 0; mode < 4; ++mode) {  // plain, masked, last_only, no session frame
        CommitSendOptions opt;
        opt.leadership_term_id = 0x0102030405060708;
        opt.cluster_session_id = -2 - mode;
        opt.last_only = mode == 2;
        opt.session_frame = mode != 3;
        std::vector<bool> ok(n, true);
        if (mode == 1)
            for (size_t i = 0; i < n; ++i) ok[i] = (i * 2654435761u >> 7) % 3 != 0;
        const std::vector<bool>* mask = mode == 1 ? &ok : nullptr;

        // the expectation, from the hand-written cases alone
        std::map<std::string, size_t> last;  // last committable record per table topic
        for (size_t i = 0; i < n; ++i)
            if (cases[i].commits) last[cases[i].topic] = i;
        std::vector<Bytes> want;
        std::vector<size_t> unsent, too_long;
        for (size_t i = 0; i < n; ++i) {
            if (!cases[i].commits || !ok[i]) continue;
            const std::string& t = cases[i].topic;
            const bool entry = std::find(table.begin(), table.end(), t) != table.end();
            if (opt.last_only && entry && last[t] != i) continue;
            const uint32_t tid = CommitManager::topic_to_id(t);
            if (tid == 0) {
                unsent.push_back(i);
            } else if (cases[i].id.size() > 65534) {
                too_long.push_back(i);
            } else {
                want.push_back(frame(opt, tid, cases[i].seq, cases[i].id, ac.message_identifier(t)));
            }
        }

        std::vector<Bytes> sent;
        size_t refused = 0;
        const OfferFn sink = [&](const std::uint8_t* p, std::size_t len) {
            sent.emplace_back(p, p + len);
            if (sent.size() % 5 == 0) {
                ++refused;
                return false;
            }
            return true;
        };
        CommitManager got, walked;
        const CommitSendResult r = ac.commit_and_send_batch(batch, got, sink, opt, mask);
        const size_t all = ac.commit_record_by_record(batch, plan, walked, mask);
        CHECK(same(got, walked));
        CHECK(mask ? r.commits == all : r.commits < all);
        CHECK(sent.size() == want.size());
        size_t bad = 0;
        for (size_t f = 0; f < sent.size() && f < want.size(); ++f) bad += sent[f] != want[f];
        if (bad) std::printf("mode %d: %zu of %zu frames differ\n", mode, bad, want.size());
        CHECK(bad == 0);
        CHECK(r.offered == sent.size() && r.accepted == sent.size() - refused);
        CHECK(r.unsent == unsent && !unsent.empty());
        CHECK(r.too_long == too_long);
        if (mode == 0) CHECK(too_long.size() == 1 && want.size() > 5 * table.size());
        if (mode == 2) CHECK(want.size() < 70);
    }

    // last_only together with a mask, and a mask of the wrong size
    {
        CommitManager cm;
        const OfferFn sink = [](const std::uint8_t*, std::size_t) { return true; };
        std::vector<bool> ok(n, true), shorter(n - 1, true);
        CommitSendOptions opt;
        opt.last_only = true;
        bool threw = false;
        try {
            ac.commit_and_send_batch(batch, cm, sink, opt, &ok);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);
        threw = false;
        try {
            ac.commit_and_send_batch(batch, cm, sink, {}, &shorter);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw && cm.get_all_commits().empty());
        // an empty batch
        const ParsedBatch none = MessageParser::decode_batch(data.data(), off.data(), 0);
        const CommitSendResult r = ac.commit_and_send_batch(none, cm, sink);
        CHECK(r.commits == 0 && r.offered == 0 && r.unsent.empty() && cm.get_all_commits().empty());
    }

    if (failures) {
        std::printf("commit send host test: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("commit send host test: ok (%zu records)\n", n);
    return 0;
}
