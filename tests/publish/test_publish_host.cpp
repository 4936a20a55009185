// OrderPublisher of the host mirror over an order file, with the message ids and TopicMessage
// timestamps of the file injected.  Modes:
//   batch  <in> <out>  publish_orders_batch: the offered records, then status and error masks
//   single <in> <out>  publish_order_to_topic per order: the offered records, then per order the
//                      outcome (0 id, 1 InvalidMessageException, 2 ClusterClientException) + text
//   misc               "Topic is empty", the default message id's format, a refused offer
#include <regex>

#include "order_file.hpp"

using namespace aeron_cluster;

struct Sink {
    std::vector<std::string> recs;
    OfferFn fn() {
        return [this](const std::uint8_t* p, std::size_t n) {
            recs.emplace_back(reinterpret_cast<const char*>(p), n);
            return true;
        };
    }
    void write(FILE* f) const {
        put_u32(f, (std::uint32_t)recs.size());
        for (const auto& r : recs) put_str(f, r);
    }
};

static OrderPublisherOptions options(const OrderFile& in, size_t* next) {
    OrderPublisherOptions o;
    o.session_framed = in.session;
    o.reference_truncate8 = in.truncate8;
    o.leadership_term_id = in.term;
    o.cluster_session_id = in.sess;
    o.message_id = [&in, next] { return in.message_ids.at(*next); };
    o.clock = [&in, next] { return in.tm_ts.at((*next)++); };  // the clock is read after the id
    return o;
}

static int misc() {
    int bad = 0;
    auto check = [&](bool ok, const char* what) {
        if (!ok) std::fprintf(stderr, "FAIL %s\n", what), ++bad;
    };
    Order o;
    o.id = "id-1";
    o.client_order_uuid = "u";
    o.base_token = "BTC";
    o.quote_token = "USDC";
    o.side = "BUY";
    o.quantity = 2.0;
    o.limit_price = 1.0;
    Sink sink;
    OrderPublisher pub(sink.fn(), "orders");
    try {
        pub.publish_order_to_topic(o, "");
        check(false, "empty topic did not throw");
    } catch (const InvalidMessageException& e) {
        check(std::string(e.what()) == "Invalid message: Topic is empty", e.what());
    }
    check(sink.recs.empty(), "nothing offered for an empty topic");
    const std::string id = pub.publish_order(o);  // default id generator and clock
    check(std::regex_match(id, std::regex("^msg_[0-9]+_[0-9]{5}$")), id.c_str());
    check(sink.recs.size() == 1 && sink.recs[0].find("\"messageId\":\"" + id + "\"") != std::string::npos,
          "the record carries the returned id");
    Order inv = o;
    inv.side = "buy";
    inv.quantity = 0.0;
    try {
        pub.publish_order(inv);
        check(false, "invalid order did not throw");
    } catch (const InvalidMessageException& e) {
        check(std::string(e.what()) == "Invalid message: Order validation failed: Side must be 'BUY' or 'SELL'",
              e.what());
    }
    OrderPublisher refuse([](const std::uint8_t*, std::size_t) { return false; }, "orders");
    try {
        refuse.publish_order(o);
        check(false, "refused offer did not throw");
    } catch (const InvalidMessageException&) {
        check(false, "refused offer threw InvalidMessageException");
    } catch (const ClusterClientException& e) {
        check(std::string(e.what()) == "Failed to publish order message", e.what());
    }
    const PublishedOrders r = refuse.publish_orders_batch({o, o});
    check(r.offered == 0 && r.status.size() == 2 && r.status[0] == 0, "batch with a refusing sink");
    if (!bad) std::puts("publish host misc: ok");
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if (mode == "misc") return misc();
        if (argc != 4) return 2;
        const OrderFile in = read_orders(argv[2]);
        FILE* out = std::fopen(argv[3], "wb");
        if (!out) return 2;
        size_t next = 0;
        Sink sink;
        OrderPublisher pub(sink.fn(), in.topic, options(in, &next));
        if (mode == "batch") {
            const PublishedOrders r = pub.publish_orders_batch(in.orders);
            sink.write(out);
            std::fwrite(r.status.data(), 1, r.status.size(), out);
            std::fwrite(r.error_mask.data(), 2, r.error_mask.size(), out);
            for (const auto& id : r.message_ids) put_str(out, id);
        } else if (mode == "single") {
            std::vector<std::pair<std::uint8_t, std::string>> res;
            for (size_t i = 0; i < in.orders.size(); ++i) {
                const Order& o = in.orders[i];
                next = i;  // order i's id and clock: an invalid order consumes neither (checked below)
                const bool valid = o.validate().empty();
                try {
                    res.emplace_back(0, pub.publish_order_to_topic(o, in.topic));
                } catch (const InvalidMessageException& e) {
                    res.emplace_back(1, e.what());
                } catch (const ClusterClientException& e) {
                    res.emplace_back(2, e.what());
                }
                // the id generator and the clock run once for a valid order and not at all for an
                // invalid one, as in the reference (validate() comes first)
                if (next != i + (valid ? 1 : 0)) {
                    std::fprintf(stderr, "order %zu: id generator / clock calls differ from the reference's\n", i);
                    return 1;
                }
            }
            sink.write(out);
            for (const auto& r : res) {
                std::fputc(r.first, out);
                put_str(out, r.second);
            }
        } else {
            return 2;
        }
        std::fclose(out);
        quiesce();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::puts("publish host: ok");
    return 0;
}
