// TEST ONLY: the host mirror's ParseResult predicates and classify_topic over hand-built
// ParseResults, for tests/test_select_lib.py to compare with the model of tests/select_lib.py.  It
// launches nothing and needs no device.
//
// File: u64 n, then per case u16 template_id, u16 schema_id, u32 type bytes, u32 payload bytes, u32
// topic bytes, and the three strings.  Output: one line per case, "<pred> <topic class>".
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "aeron_cluster_amd.hpp"
#include "sbecodec.h"

using namespace aeron_cluster;

int main(int argc, char** argv) {
    if (argc < 2) return 64;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n = 0;
    if (std::fread(&n, 8, 1, f) != 1) return 3;
    for (uint64_t i = 0; i < n; ++i) {
        uint16_t ids[2];
        uint32_t len[3];
        if (std::fread(ids, 2, 2, f) != 2 || std::fread(len, 4, 3, f) != 3) return 4;
        std::string s[3];
        for (int k = 0; k < 3; ++k) {
            s[k].resize(len[k]);
            if (len[k] && std::fread(s[k].data(), 1, len[k], f) != len[k]) return 5;
        }
        ParseResult r;
        r.success = true;
        r.template_id = ids[0];
        r.schema_id = ids[1];
        r.message_type = s[0];
        r.payload = s[1];
        const unsigned pred = (r.is_session_event() ? SBE_PR_SESSION_EVENT : 0u) | (r.is_topic_message() ? SBE_PR_TOPIC_MESSAGE : 0u) |
                              (r.is_acknowledgment() ? SBE_PR_ACKNOWLEDGMENT : 0u) | (r.is_order_message() ? SBE_PR_ORDER_MESSAGE : 0u);
        const TopicClass tc = classify_topic(s[2]);
        std::printf("%u %u\n", pred, tc == TopicClass::Orders ? SBE_TC_ORDERS : tc == TopicClass::Control ? SBE_TC_CONTROL : SBE_TC_UNKNOWN);
    }
    std::fclose(f);
    return 0;
}
