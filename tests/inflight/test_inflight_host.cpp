// AckCorrelator and TopicPublisher::set_correlator of the host mirror against a plain
// std::unordered_map run of the same sequence (ClusterClient::remember_outgoing / on_ack_default,
// src/cluster_client.cpp:1920-1941).  Prints "inflight host: ok" and exits 0 when every result
// agrees.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "aeron_cluster_amd.hpp"

using namespace aeron_cluster;

namespace {
int g_bad = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c) && g_bad++ < 20) std::printf("line %d: %s\n", __LINE__, #c); \
    } while (0)

struct Ref {  // the reference's two functions on its own container
    std::unordered_map<std::string, std::uint64_t> inflight;
    void remember_outgoing(const std::string& uuid, std::uint64_t ts) { inflight.emplace(uuid, ts); }
    AckMatch on_ack(const AckInfo& ack, std::uint64_t now) {
        auto it = !ack.message_id.empty() ? inflight.find(ack.message_id) : inflight.end();
        if (it != inflight.end()) {
            const auto send_ns = it->second;
            inflight.erase(it);
            return {true, (std::int64_t)now - (std::int64_t)send_ns};
        }
        return {false, (std::int64_t)now - (std::int64_t)ack.timestamp_nanos};
    }
};

void put16(std::string& s, std::size_t v) {
    s.push_back((char)(v & 0xff));
    s.push_back((char)(v >> 8));
}
// a full ack (blockLength 8, template 2, schema 1) with the eight spare bytes decode_ack's
// len - 8 wrap needs; ts is nanoseconds already (above the decoder's unit heuristics)
std::string full_ack(const std::string& id, std::uint64_t ts) {
    std::string s;
    put16(s, 8), put16(s, 2), put16(s, 1), put16(s, 1);
    s.append(reinterpret_cast<const char*>(&ts), 8);
    for (const std::string* f : {&id, (const std::string*)nullptr}) {
        const std::string v = f ? *f : std::string("orders");
        put16(s, v.size());
        s += v;
    }
    put16(s, 1);
    s += "c";
    s.append(8, '\0');
    return s;
}
std::string simple_ack(std::uint64_t ts) {
    std::string s;
    put16(s, 8), put16(s, 2), put16(s, 1), put16(s, 1);
    s.append(reinterpret_cast<const char*>(&ts), 8);
    return s;
}
bool same(const AckMatch& a, const AckMatch& b) { return a.matched == b.matched && a.rtt_ns == b.rtt_ns; }
}  // namespace

int main() {
    std::mt19937_64 rng(99);
    const std::uint64_t T0 = 1'760'000'000'000'000'000ull;
    // the key pool: publish_topic uuids, short keys, keys of 40, 41 and 60 bytes, the empty key
    std::vector<std::string> pool{"", "a", std::string("a\0", 2), std::string(40, 'x'), std::string(41, 'x'),
                                  std::string(60, 'y'), std::string(41, 'x') + "z"};
    for (int i = 0; i < 600; ++i) pool.push_back("pub_" + std::to_string(T0 + rng() % 100000));
    AckCorrelator cor(64, 1);  // 64 slots: the sequence below forces growth by rehash
    Ref ref;
    CHECK(cor.capacity() == 64 && cor.rehashes() == 0);

    // single forms, keys of every kind
    for (int i = 0; i < 40; ++i) {
        const std::string& k = pool[i % 12];
        cor.remember_outgoing(k, T0 + i);
        ref.remember_outgoing(k, T0 + i);
    }
    CHECK(cor.size() == ref.inflight.size());
    for (int i = 0; i < 16; ++i) {
        AckInfo a;
        a.message_id = pool[(i * 5) % 14];
        a.timestamp_nanos = T0 + 1000 + i;
        CHECK(same(cor.on_ack(a, T0 + 5000), ref.on_ack(a, T0 + 5000)));
    }
    CHECK(cor.size() == ref.inflight.size());

    // batch forms: remember, then acks as wire records through the device decode
    std::uint64_t acks_seen = 0, matched = 0;
    for (int round = 0; round < 12; ++round) {
        std::vector<std::string> uuids;
        std::vector<std::uint64_t> ts;
        const int n = 50 + (int)(rng() % 200);
        for (int i = 0; i < n; ++i) {
            uuids.push_back(pool[rng() % pool.size()]);
            ts.push_back(T0 + rng() % 1000000);
        }
        cor.remember_batch(uuids, ts);
        for (int i = 0; i < n; ++i) ref.remember_outgoing(uuids[i], ts[i]);
        CHECK(cor.size() == ref.inflight.size());

        std::string data(5, '\xEE');  // the batch need not start at offset 0
        std::vector<std::uint64_t> off{data.size()};
        std::vector<AckInfo> infos;  // what MessageHandler would hand on_ack_default per ack
        const int m = 30 + (int)(rng() % 150);
        for (int i = 0; i < m; ++i) {
            const int kind = (int)(rng() % 10);
            const std::uint64_t ats = T0 + 2000000 + rng() % 1000;
            if (kind == 0) {
                data += simple_ack(ats);
                AckInfo a;
                a.timestamp_nanos = ats;
                a.simple_control_ack = true;
                infos.push_back(a);
            } else if (kind == 1) {
                data += std::string("\x01\x02\x03", 3);  // undecodable: no callback
            } else {
                AckInfo a;
                a.message_id = pool[rng() % pool.size()];
                a.timestamp_nanos = ats;
                data += full_ack(a.message_id, ats);
                infos.push_back(a);
            }
            off.push_back(data.size());
        }
        const std::uint64_t now = T0 + 9000000;
        const auto got = cor.on_egress_batch(reinterpret_cast<const std::uint8_t*>(data.data()), off.data(), off.size() - 1, now);
        CHECK(got.size() == infos.size());
        for (std::size_t i = 0; i < infos.size() && i < got.size(); ++i) {
            const AckMatch e = ref.on_ack(infos[i], now);
            CHECK(same(got[i], e));
            ++acks_seen;
            matched += e.matched;
        }
        CHECK(cor.size() == ref.inflight.size());
    }
    CHECK(acks_seen > 500 && matched > 100);
    CHECK(cor.rehashes() >= 2 && cor.capacity() > 64);

    // TopicPublisher with a sink that refuses every third offer: exactly the accepted records are remembered
    {
        AckCorrelator pc(64);
        int offers = 0;
        std::vector<std::string> accepted_bytes;
        TopicPublisher pub([&](const std::uint8_t* p, std::size_t len) {
            const bool ok = ++offers % 3 != 0;
            if (ok) accepted_bytes.emplace_back(reinterpret_cast<const char*>(p), len);
            return ok;
        });
        std::vector<TopicMessageFields> msgs(40);
        for (auto& f : msgs) f = TopicMessageFields{"orders", "CREATE_ORDER", {}, "{\"q\":1}", {}, 0};
        const auto quiet = pub.publish_topic_batch(msgs);  // no correlator yet: nothing remembered
        CHECK(pc.size() == 0);
        pub.set_correlator(&pc);
        offers = 0;
        accepted_bytes.clear();
        auto uuids = pub.publish_topic_batch(msgs);
        uuids.push_back(pub.publish_topic("orders", "CREATE_ORDER", "{}", ""));  // offer 41: accepted
        uuids.push_back(pub.publish_topic("orders", "CREATE_ORDER", "{}", ""));  // offer 42: refused
        CHECK(offers == 42);
        std::unordered_map<std::string, std::uint64_t> want;  // uuid -> the timestamp inside the accepted record
        std::size_t k = 0;
        for (int i = 0; i < 42; ++i) {
            if ((i + 1) % 3 == 0) continue;
            std::uint64_t ts;
            std::memcpy(&ts, accepted_bytes[k++].data() + 8, 8);
            want.emplace(uuids[i], ts);
        }
        CHECK(pc.size() == want.size());
        for (int i = 0; i < 42; ++i) {
            AckInfo a;
            a.message_id = uuids[i];
            a.timestamp_nanos = 77;
            const AckMatch g = pc.on_ack(a, T0);
            auto it = want.find(uuids[i]);
            if (it != want.end()) {
                CHECK(g.matched && g.rtt_ns == (std::int64_t)T0 - (std::int64_t)it->second);
                want.erase(it);  // a uuid drawn twice in one nanosecond matches once
            } else {
                CHECK(!g.matched && g.rtt_ns == (std::int64_t)T0 - 77);
            }
        }
        CHECK(pc.size() == 0);
    }
    if (g_bad) {
        std::printf("inflight host: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("inflight host: ok (%llu acks, %llu matched, capacity %llu after %llu rehashes)\n",
                (unsigned long long)acks_seen, (unsigned long long)matched, (unsigned long long)cor.capacity(),
                (unsigned long long)cor.rehashes());
    return 0;
}
