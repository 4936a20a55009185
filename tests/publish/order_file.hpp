// The order file the Python tests write (publish_lib.write_orders), little endian:
//   u32 n, u8 session_framed, u8 reference_truncate8, i64 leadership_term_id, i64 cluster_session_id,
//   string topic; per order: strings client_order_uuid, identifier, base_token, quote_token, side,
//   id, message_id, status, order_type, time_in_force; f64 quantity, i64 customer_id,
//   i64 timestamp, f64 limit_price, f64 stop_price, u8 present (bit 0 stop_price, bit 1
//   expiry_timestamp), u64 TopicMessage timestamp.   string = u32 length + bytes.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "aeron_cluster_amd.hpp"

struct OrderFile {
    bool session = true, truncate8 = true;
    std::int64_t term = 0, sess = 0;
    std::string topic;
    std::vector<aeron_cluster::Order> orders;
    std::vector<std::string> message_ids;
    std::vector<std::uint64_t> tm_ts;
};

class Reader {
public:
    explicit Reader(const char* path) {
        FILE* f = std::fopen(path, "rb");
        if (!f) throw std::runtime_error(std::string("cannot open ") + path);
        std::uint8_t buf[65536];
        for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) d_.insert(d_.end(), buf, buf + k);
        std::fclose(f);
    }
    template <class T>
    T get() {
        if (at_ + sizeof(T) > d_.size()) throw std::runtime_error("order file: short");
        T v;
        std::memcpy(&v, d_.data() + at_, sizeof(T));
        at_ += sizeof(T);
        return v;
    }
    std::string str() {
        const std::uint32_t n = get<std::uint32_t>();
        if (at_ + n > d_.size()) throw std::runtime_error("order file: short string");
        std::string s(reinterpret_cast<const char*>(d_.data() + at_), n);
        at_ += n;
        return s;
    }

private:
    std::vector<std::uint8_t> d_;
    size_t at_ = 0;
};

inline OrderFile read_orders(const char* path) {
    Reader r(path);
    OrderFile f;
    const std::uint32_t n = r.get<std::uint32_t>();
    f.session = r.get<std::uint8_t>() != 0;
    f.truncate8 = r.get<std::uint8_t>() != 0;
    f.term = r.get<std::int64_t>();
    f.sess = r.get<std::int64_t>();
    f.topic = r.str();
    for (std::uint32_t i = 0; i < n; ++i) {
        aeron_cluster::Order o;
        o.client_order_uuid = r.str();
        o.identifier = r.str();
        o.base_token = r.str();
        o.quote_token = r.str();
        o.side = r.str();
        o.id = r.str();
        f.message_ids.push_back(r.str());
        o.status = r.str();
        o.order_type = r.str();
        o.time_in_force = r.str();
        o.quantity = r.get<double>();
        o.customer_id = r.get<std::int64_t>();
        o.timestamp = r.get<std::int64_t>();
        o.limit_price = r.get<double>();
        const double stop = r.get<double>();
        const std::uint8_t present = r.get<std::uint8_t>();
        if (present & 1) o.stop_price = stop;
        if (present & 2) o.expiry_timestamp = 1;
        f.tm_ts.push_back(r.get<std::uint64_t>());
        f.orders.push_back(std::move(o));
    }
    return f;
}

inline void put_u32(FILE* f, std::uint32_t v) { std::fwrite(&v, 4, 1, f); }
inline void put_str(FILE* f, const std::string& s) {
    put_u32(f, (std::uint32_t)s.size());
    if (!s.empty()) std::fwrite(s.data(), 1, s.size(), f);
}
