// AutoCommitter (host mirror) against the reference's sequence, record by record: a batch whose
// commit decisions and topic texts are written out by hand is committed (1) by a plain loop over
// those expectations, (2) by AutoCommitter::commit_batch without a mask (one commit per topic-table
// entry plus the unresolved records), (3) with a callback mask; the CommitManager states must be
// equal.  The device plan is also compared with the restatement (commit_ref.cpp) on the same
// descriptors.  Needs a GPU (run by tests/test_gpu_autocommit.py).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "aeron_cluster_amd.hpp"
#include "sbecodec.h"

using namespace aeron_cluster;

extern "C" void cref_classify(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const uint8_t* status,
                              const uint8_t* flags, const uint32_t* view_off, const uint32_t* view_len,
                              const uint8_t* tarena, const uint32_t* toff, uint32_t k, uint8_t* cm, uint8_t* src,
                              uint8_t* kind, uint32_t* off, uint32_t* len, uint32_t* idx, uint64_t* last,
                              uint64_t* count);

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static void put_str(std::vector<uint8_t>& b, const std::string& s) {
    b.push_back((uint8_t)(s.size() & 0xff));
    b.push_back((uint8_t)(s.size() >> 8));
    b.insert(b.end(), s.begin(), s.end());
}
static std::vector<uint8_t> tm_wire(const std::string& type, const std::string& id, const std::string& payload,
                                    const std::string& headers, uint64_t ts) {
    std::vector<uint8_t> b = {16, 0, 1, 0, 1, 0, 1, 0};
    for (int k = 0; k < 8; ++k) b.push_back((uint8_t)(ts >> (8 * k)));
    for (int k = 0; k < 8; ++k) b.push_back(0);
    put_str(b, "orders");
    put_str(b, type);
    put_str(b, id);
    put_str(b, payload);
    put_str(b, headers);
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
    std::vector<Case> base = {
        {"CREATE_ORDER", "m1", P, "{}", true, "orders", 0},
        {"CREATE_ORDER", "m2", "{\"_sequence_number\":41}", "{\"topic\":\"alpha\"}", true, "alpha", 41},
        {"X", "m3", "{\"topic\":\"beta\",\"_sequence_number\":\"7\"}", "", true, "beta", 7},
        {"X", "m4", "{\"message\":{\"topic\":\"gamma\"}}", "{}", true, "gamma", 0},              // not in the table
        {"X", "m5", P, "{\"topic\":\"\\u0061lpha\"}", true, "alpha", 0},                          // escaped
        {"X", "m6", P, "{\"topic\":\"g\\u0061mm\\\"a\\n\"}", true, "gamm\"a\n", 0},               // escaped, unknown
        {"X", "m7", P, "{\"topic\":12}", true, "12", 0},                                          // Value::asString
        {"X", "m8", P, "{\"topic\":-0}", true, "0", 0},
        {"X", "m9", P, "{\"topic\":1.5}", true, "1.5", 0},
        {"X", "m10", P, "{\"topic\":1e2}", true, "100.0", 0},
        {"X", "m11", P, "{\"topic\":18446744073709551616}", true, "1.8446744073709552e+19", 0},
        {"X", "m12", P, "{\"topic\":true}", true, "true", 0},
        {"X", "m13", P, "{\"topic\":null}", true, "", 0},
        {"X", "m14", P, "{\"topic\":\"a:b\"}", true, "a:b", 0},   // "a:b" + ":" + client collides with ...
        {"X", "m15", P, "{\"topic\":\"a\"}", true, "a", 0},       // ... "a" + ":" + "b:cli" below
        {"SUBSCRIBE", "m16", P, "{\"topic\":\"alpha\"}", false, "", 0},
        {"X", "ack_17", P, "{\"topic\":\"alpha\"}", false, "", 0},
        {"X", "m18", P, "{\"topic\":\"_ack\"}", false, "", 0},
        {"X", "m19", P, "{\"topic\":\"_control\"}", false, "", 0},
        {"REPLAY_COMPLETE", "m20", "", "{\"topic\":\"_control\"}", true, "_control", 0},
        {"X", "m21", "", "{}", false, "", 0},
        {"X", "", P, "{}", false, "", 0},
        {"X", "m23", P, "{\"topic\":[1]}", true, "orders", 0},
    };
    // several rounds in rotated order, so that the last commit per key is not always the same case
    std::vector<Case> cases;
    for (int round = 0; round < 9; ++round)
        for (size_t j = 0; j < base.size(); ++j) {
            Case c = base[(j * 5 + round * 7) % base.size()];
            if (!c.id.empty() && c.id.compare(0, 4, "ack_") != 0) c.id += "_r" + std::to_string(round);
            cases.push_back(c);
        }
    std::vector<uint8_t> data;
    std::vector<uint64_t> off = {0};
    for (size_t i = 0; i < cases.size(); ++i) {
        const auto r = tm_wire(cases[i].type, cases[i].id, cases[i].payload, cases[i].headers, 1000 + i);
        data.insert(data.end(), r.begin(), r.end());
        off.push_back(data.size());
        if (i % 11 == 0) {  // an unparsed record in between
            data.push_back(1);
            off.push_back(data.size());
            cases.insert(cases.begin() + i + 1, Case{"", "", "", "", false, "", 0});
            ++i;
        }
    }
    const size_t n = cases.size();
    CHECK(off.size() == n + 1);

    AutoCommitter ac("cli", "orders");
    ac.set_message_identifier("alpha", "id-alpha");
    ac.set_message_identifier("beta", "id-beta");
    ac.set_message_identifier("a", "b:cli");
    ac.set_message_identifier("never", "id-never");
    CHECK(ac.message_identifier("alpha") == "id-alpha" && ac.message_identifier("zzz") == "cli");

    const ParsedBatch batch = MessageParser::decode_batch(data.data(), off.data(), n);
    // the decode this test builds on: every record's message_id view before anything is classified
    // (a mismatch here is the decode's, not the classification's)
    size_t decode_bad = 0;
    for (size_t i = 0; i < n; ++i)
        if (off[i + 1] - off[i] > 1 && std::string(batch.view(i, 2)) != cases[i].id) ++decode_bad;
    if (decode_bad) std::printf("decode_batch: %zu of %zu message_id views differ from the records\n", decode_bad, n);
    CHECK(decode_bad == 0);
    const CommitPlan plan = ac.classify(batch);
    CHECK(plan.table.size() == 5 && plan.table[0] == "orders");

    // the device plan against the restatement, on the same descriptors
    {
        std::vector<uint8_t> st(n), fl(n), cm(n), src(n), kind(n), arena(SBE_COMMIT_TABLE_BYTES, 0);
        std::vector<uint32_t> vo(5 * n), vl(5 * n), to(plan.table.size() + 1, 0), o(n), l(n), idx(n);
        std::vector<uint64_t> last(plan.table.size()), count(plan.table.size() + 2);
        for (size_t i = 0; i < n; ++i) {
            st[i] = batch.status(i);
            for (int f = 0; f < 5; ++f) {
                const std::string_view v = batch.view(i, f);
                vl[5 * i + f] = (uint32_t)v.size();
                vo[5 * i + f] = v.data() ? (uint32_t)(reinterpret_cast<const uint8_t*>(v.data()) - (data.data() + off[i])) : 0;
            }
        }
        for (size_t j = 0; j < plan.table.size(); ++j) {
            std::memcpy(arena.data() + to[j], plan.table[j].data(), plan.table[j].size());
            to[j + 1] = to[j] + (uint32_t)plan.table[j].size();
        }
        cref_classify(data.data(), off.data(), n, st.data(), fl.data(), vo.data(), vl.data(), arena.data(), to.data(),
                      (uint32_t)plan.table.size(), cm.data(), src.data(), kind.data(), o.data(), l.data(), idx.data(),
                      last.data(), count.data());
        CHECK(cm == plan.cm && src == plan.topic_src && kind == plan.topic_kind && o == plan.topic_off &&
              l == plan.topic_len && idx == plan.topic_idx && last == plan.last && count == plan.count);
    }

    size_t commits = 0;
    for (size_t i = 0; i < n; ++i) {
        if ((plan.cm[i] == SBE_CM_COMMIT) != cases[i].commits)
            std::printf("record %zu: status %u cm %u src %u idx %u, expected commits=%d, id '%s' view id '%s'\n", i,
                        (unsigned)batch.status(i), (unsigned)plan.cm[i], (unsigned)plan.topic_src[i],
                        (unsigned)plan.topic_idx[i], (int)cases[i].commits, cases[i].id.c_str(),
                        std::string(batch.view(i, 2)).c_str());
        CHECK((plan.cm[i] == SBE_CM_COMMIT) == cases[i].commits);
        if (cases[i].commits) {
            CHECK(ac.topic(batch, plan, i) == cases[i].topic);
            CHECK(batch.sequence_number(i) == cases[i].seq);
            ++commits;
        }
    }

    for (int masked = 0; masked < 2; ++masked) {
        std::vector<bool> ok(n, true);
        if (masked)
            for (size_t i = 0; i < n; ++i) ok[i] = (i * 2654435761u >> 7) % 3 != 0;
        // (1) the reference's sequence from the hand-written expectations
        CommitManager expect;
        for (size_t i = 0; i < n; ++i)
            if (cases[i].commits && ok[i])
                expect.commit_message(cases[i].topic, ac.message_identifier(cases[i].topic), cases[i].id, 1000 + i,
                                      cases[i].seq);
        // (2) / (3) the AutoCommitter
        CommitManager got, walked;
        const size_t calls = ac.commit_batch(batch, plan, got, masked ? &ok : nullptr);
        const size_t all = ac.commit_record_by_record(batch, plan, walked, masked ? &ok : nullptr);
        CHECK(same(got, walked));
        CHECK(same(walked, expect));
        if (!masked) {
            CHECK(all == commits);
            CHECK(calls < all);  // one call per table entry, not per record
            CommitManager direct;
            CHECK(ac.commit_batch(batch, direct) == calls && same(direct, expect));
        }
        CHECK(got.get_last_commit("never", "id-never") == nullptr);
        const auto a = got.get_last_commit("alpha", "id-alpha");
        CHECK(a && a->topic == "alpha" && a->message_identifier == "id-alpha");
    }

    // an empty batch
    const ParsedBatch none = MessageParser::decode_batch(data.data(), off.data(), 0);
    CommitManager empty;
    CHECK(ac.commit_batch(none, empty) == 0 && empty.get_all_commits().empty());

    if (failures) {
        std::printf("autocommit host test: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("autocommit host test: ok (%zu records, %zu commits)\n", n, commits);
    return 0;
}
