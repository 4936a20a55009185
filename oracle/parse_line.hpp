// parse_line.hpp — TEST INFRASTRUCTURE ONLY: one canonical text line per record from the
// aeron_cluster API (ParseResult, MessageParser, SBEUtils), written against the names alone so that
// the same text comes out of two implementations: oracle/ref_sources.cpp compiles it against the
// reference's headers, tests/cpp/test_parse_lines.cpp against the host mirror's.  Include it after
// the header that declares aeron_cluster::ParseResult.  Strings are printed as hex.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace parse_line {

inline std::string hex(const std::string& s) {
    static const char* d = "0123456789abcdef";
    std::string o;
    o.reserve(2 * s.size() + 1);
    for (unsigned char c : s) {
        o += d[c >> 4];
        o += d[c & 15];
    }
    return o.empty() ? "-" : o;
}

// every ParseResult field, the four predicates, and the host-side helpers that take a result
inline std::string of_result(const aeron_cluster::ParseResult& r) {
    char num[512];
    std::snprintf(num, sizeof num,
                  " ts=%lld seq=%llu tmpl=%u schema=%u ver=%u blk=%u corr=%lld sess=%lld leader=%d code=%d term=%lld"
                  " pred=%d%d%d%d",
                  (long long)r.timestamp, (unsigned long long)r.sequence_number, (unsigned)r.template_id,
                  (unsigned)r.schema_id, (unsigned)r.version, (unsigned)r.block_length, (long long)r.correlation_id,
                  (long long)r.session_id, (int)r.leader_member_id, (int)r.event_code, (long long)r.leadership_term_id,
                  (int)r.is_session_event(), (int)r.is_topic_message(), (int)r.is_acknowledgment(),
                  (int)r.is_order_message());
    return std::string("ok=") + (r.success ? "1" : "0") + " err=" + hex(r.error_message) + " type=" + hex(r.message_type) +
           " id=" + hex(r.message_id) + " payload=" + hex(r.payload) + " headers=" + hex(r.headers) + num +
           " desc=" + hex(r.get_description()) +
           " tname=" + hex(aeron_cluster::SBEUtils::get_message_type_name(r.template_id, r.schema_id)) +
           " codes=" + hex(aeron_cluster::SBEUtils::get_session_event_code_string(r.event_code));
}

// the helpers that read the record's bytes alone
inline std::string of_bytes(const std::uint8_t* data, std::size_t len) {
    namespace ac = aeron_cluster;
    std::int32_t code = (std::int32_t)len;  // a record too short for a SessionEvent: its length, for variety
    if (len >= 40) std::memcpy(&code, data + 36, 4);
    std::string s = "mtype=" + hex(ac::MessageParser::get_message_type(data, len)) +
                    " corrid=" + std::to_string((long long)ac::MessageParser::extract_correlation_id(data, len)) +
                    " valid=" + (ac::SBEUtils::is_valid_sbe_message(data, len) ? "1" : "0") +
                    " rawcode=" + hex(ac::SBEUtils::get_session_event_code_string(code)) + " strings=";
    const std::vector<std::string> runs = ac::SBEUtils::extract_readable_strings(data, len, 3);
    for (std::size_t k = 0; k < runs.size(); ++k) s += (k ? "," : "") + hex(runs[k]);
    if (runs.empty()) s += "-";
    s += " strings5=" + std::to_string(ac::SBEUtils::extract_readable_strings(data, len, 5).size());
    return s;
}

// is_acknowledgment_for with the record's own message id, a part of it, and a text it cannot hold
inline std::string of_ack_for(const std::uint8_t* data, std::size_t len, const std::string& own_id) {
    namespace ac = aeron_cluster;
    const std::string part = own_id.size() > 2 ? own_id.substr(1, own_id.size() - 2) : own_id;
    return std::string("ackfor=") + (ac::MessageParser::is_acknowledgment_for(data, len, own_id) ? "1" : "0") +
           (ac::MessageParser::is_acknowledgment_for(data, len, part) ? "1" : "0") +
           (ac::MessageParser::is_acknowledgment_for(data, len, "\x01no-such-id\x02") ? "1" : "0");
}

}  // namespace parse_line
