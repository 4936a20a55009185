// Order::validate() of the host mirror (src/order_types.cpp:66-120) over an order file: writes,
// per order, u32 count and the message strings.  Also checks the defaults of a fresh Order
// (order_types.hpp:28-49).  Host code only: no device call is made.
#include "order_file.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    try {
        const aeron_cluster::Order d;
        if (d.order_type != "LIMIT" || d.time_in_force != "GTC" || d.limit_price != 0.0 || d.stop_price.has_value() ||
            d.expiry_timestamp.has_value() || d.status != "CREATED" || d.quantity != 0.0) {
            std::fprintf(stderr, "Order defaults differ from order_types.hpp:28-49\n");
            return 1;
        }
        const OrderFile in = read_orders(argv[1]);
        FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 2;
        // the all-defaults Order first, then the file's
        std::vector<aeron_cluster::Order> all{d};
        all.insert(all.end(), in.orders.begin(), in.orders.end());
        for (const auto& o : all) {
            const std::vector<std::string> e = o.validate();
            put_u32(out, (std::uint32_t)e.size());
            for (const auto& m : e) put_str(out, m);
        }
        std::fclose(out);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::puts("order validate: ok");
    return 0;
}
