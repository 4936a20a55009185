// AutoCommitter::commit_and_send_batch with CommitSendOptions::json_fallback (host mirror): a batch
// whose commit decisions and topic texts are written out by hand is committed and sent.  The sink
// must receive every frame in record order: the CommitOffsetLite of topics with an id, and for
// topics without one the JSON TopicMessage, which the device builds for table entries and plain
// string topics and the host builds for escaped and non-string topics.  Every JSON frame is
// compared with CommitManager::build_commit_offset_fallback on the same offset and clock readings
// (that function is checked against the reference's rules without a GPU by
// tests/test_commit_fallback_host.py), so device-built and host-built frames of the same kind of
// record are identical.  `unsent` stays empty, records over the 1040-byte bound land in
// `fallback_e100`, and with the option off the call behaves as before.  Needs a GPU (run by
// tests/test_gpu_commit_fallback_host.py).
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
static Bytes session_header(const CommitSendOptions& o) {
    Bytes b;
    if (!o.session_frame) return b;
    for (uint16_t v : {24, 1, 111, 8}) put_le(b, v, 2);
    put_le(b, (uint64_t)o.leadership_term_id, 8);
    put_le(b, (uint64_t)o.cluster_session_id, 8);
    put_le(b, 0, 8);
    return b;
}
static Bytes lite_frame(const CommitSendOptions& o, uint32_t tid, uint64_t seq, const std::string& id,
                        const std::string& ident) {
    Bytes b = session_header(o);
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
    bool device;        // a JSON frame of this record is built on the device (else on the host)
};

static const uint64_t kNow = 1700000000123456789ull, kUuid = 1700000000999999000ull;

int main() {
    const std::string P = "{\"x\":1}";
    const std::vector<Case> base = {
        {"CREATE_ORDER", "m1", P, "{}", true, "mine", 0, true},                                    // the fallback entry, id 0
        {"X", "m2", "{\"_sequence_number\":41}", "{\"topic\":\"order_notification_topic\"}", true, "order_notification_topic", 41, true},
        {"X", "m3\"\x01\xc3\xa9", P, "{\"topic\":\"alpha\"}", true, "alpha", 0, true},                // a table entry with id 0
        {"X", "m4", "{\"topic\":\"order_request_topic\",\"_sequence_number\":\"7\"}", "", true, "order_request_topic", 7, true},  // not in the table, id 1
        {"X", "m5", P, "{\"topic\":\"order_\\u0072equest_topic\"}", true, "order_request_topic", 0, false},  // the same, escaped
        {"X", "m6", "{\"_sequence_number\":5}", "{\"topic\":\"gamma\"}", true, "gamma", 5, true},    // unknown plain topic
        {"X", "m7", P, "{\"topic\":\"g\\u0061mma\"}", true, "gamma", 0, false},                     // unknown escaped topic: host
        {"X", "m8", P, "{\"topic\":12}", true, "12", 0, false},                                     // Value::asString: host
        {"X", "m9", P, "{\"topic\":\"orders\"}", true, "orders", 0, true},                           // id 3, not in the table
        {"SUBSCRIBE", "m10", P, "{}", false, "", 0, true},
        {"X", "ack_11", P, "{}", false, "", 0, true},
        {"X", "", P, "{}", false, "", 0, true},
    };
    std::vector<Case> cases;
    for (int round = 0; round < 9; ++round)
        for (size_t j = 0; j < base.size(); ++j) {
            Case c = base[(j * 5 + round * 7) % base.size()];
            if (!c.id.empty() && c.id.compare(0, 4, "ack_") != 0) c.id += "_r" + std::to_string(round);
            cases.push_back(c);
        }
    cases.insert(cases.begin() + 30, Case{"X", std::string(1500, 'L'), P, "{\"topic\":\"gamma\"}", true, "gamma", 0, true});        // E100, device
    cases.insert(cases.begin() + 60, Case{"X", std::string(1500, 'M'), P, "{\"topic\":\"g\\u0061mma\"}", true, "gamma", 0, false});  // E100, host
    cases.insert(cases.begin() + 80, Case{"X", std::string(65535, 'N'), P, "{\"topic\":\"orders\"}", true, "orders", 0, true});     // E109
    Bytes data;
    std::vector<uint64_t> off = {0};
    for (size_t i = 0; i < cases.size(); ++i) {
        const Bytes r = tm_wire(cases[i].type, cases[i].id, cases[i].payload, cases[i].headers, 1000 + i);
        data.insert(data.end(), r.begin(), r.end());
        off.push_back(data.size());
    }
    const size_t n = cases.size();

    AutoCommitter ac("cli-\xc3\xa9", "mine");
    ac.set_message_identifier("order_notification_topic", "id-notif");
    ac.set_message_identifier("alpha", "id-\"alpha\"");
    const std::vector<std::string> table = {"mine", "alpha", "order_notification_topic"};

    const ParsedBatch batch = MessageParser::decode_batch(data.data(), off.data(), n);
    const CommitPlan plan = ac.classify(batch);
    CHECK(plan.table == table);
    for (size_t i = 0; i < n; ++i) {
        CHECK((plan.cm[i] == SBE_CM_COMMIT) == cases[i].commits);
        if (cases[i].commits) CHECK(ac.topic(batch, plan, i) == cases[i].topic && batch.sequence_number(i) == cases[i].seq);
    }

    const CommitManager builder;
    for (int mode = 0; mode < 5; ++mode) {  // plain, masked, last_only, no session frame, the option off
        CommitSendOptions opt;
        opt.leadership_term_id = 0x0102030405060708;
        opt.cluster_session_id = -2 - mode;
        opt.last_only = mode == 2;
        opt.session_frame = mode != 3;
        opt.json_fallback = mode != 4;
        int reads = 0;
        opt.clock = [&] { return reads++ ? kUuid : kNow; };
        std::vector<bool> ok(n, true);
        if (mode == 1)
            for (size_t i = 0; i < n; ++i) ok[i] = (i * 2654435761u >> 7) % 3 != 0;
        const std::vector<bool>* mask = mode == 1 ? &ok : nullptr;

        // the expectation, from the hand-written cases alone
        std::map<std::string, size_t> last;
        for (size_t i = 0; i < n; ++i)
            if (cases[i].commits) last[cases[i].topic] = i;
        std::vector<Bytes> want;
        std::vector<size_t> unsent, too_long, e100;
        size_t json_device = 0, json_host = 0;
        for (size_t i = 0; i < n; ++i) {
            if (!cases[i].commits || !ok[i]) continue;
            const std::string& t = cases[i].topic;
            const bool entry = std::find(table.begin(), table.end(), t) != table.end();
            if (opt.last_only && entry && last[t] != i) continue;
            const uint32_t tid = CommitManager::topic_to_id(t);
            if (tid != 0) {
                if (cases[i].id.size() > 65534) too_long.push_back(i);
                else want.push_back(lite_frame(opt, tid, cases[i].seq, cases[i].id, ac.message_identifier(t)));
                continue;
            }
            if (!opt.json_fallback) {
                unsent.push_back(i);
                continue;
            }
            const CommitOffset o{t, ac.message_identifier(t), cases[i].id, 1000 + i, cases[i].seq};
            int r2 = 0;
            try {
                const Bytes rec = builder.build_commit_offset_fallback(o.message_identifier, o,
                                                                       [&] { return r2++ ? kUuid + i : kNow; });
                Bytes f = session_header(opt);
                f.insert(f.end(), rec.begin(), rec.end());
                want.push_back(f);
                ++(cases[i].device ? json_device : json_host);
            } catch (const std::runtime_error&) {
                e100.push_back(i);
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
        ac.commit_record_by_record(batch, plan, walked, mask);
        CHECK(reads == (opt.json_fallback ? 2 : 0));
        CHECK(sent.size() == want.size());
        size_t bad = 0;
        for (size_t f = 0; f < sent.size() && f < want.size(); ++f) bad += sent[f] != want[f];
        if (bad) std::printf("mode %d: %zu of %zu frames differ\n", mode, bad, want.size());
        CHECK(bad == 0);
        CHECK(r.offered == sent.size() && r.accepted == sent.size() - refused);
        CHECK(r.unsent == unsent && r.too_long == too_long && r.fallback_e100 == e100);
        CHECK(r.unsent.empty() == opt.json_fallback);
        if (mode == 0) CHECK(json_device > 20 && json_host > 10 && e100.size() == 2 && too_long.size() == 1);
        if (mode == 4) CHECK(e100.empty() && unsent.size() > 30);
        // the commits are the same whatever is sent
        const auto x = got.get_all_commits(), y = walked.get_all_commits();
        CHECK(x.size() == y.size());
        for (const auto& kv : x) {
            auto it = y.find(kv.first);
            CHECK(it != y.end() && it->second.message_id == kv.second.message_id &&
                  it->second.sequence_number == kv.second.sequence_number);
        }
    }

    {  // an empty batch with the option on
        CommitManager cm;
        CommitSendOptions opt;
        opt.json_fallback = true;
        const OfferFn sink = [](const std::uint8_t*, std::size_t) { return true; };
        const ParsedBatch none = MessageParser::decode_batch(data.data(), off.data(), 0);
        const CommitSendResult r = ac.commit_and_send_batch(none, cm, sink, opt);
        CHECK(r.commits == 0 && r.offered == 0 && r.unsent.empty() && r.fallback_e100.empty());
    }

    if (failures) {
        std::printf("fallback send host test: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("fallback send host test: ok (%zu records)\n", n);
    return 0;
}
