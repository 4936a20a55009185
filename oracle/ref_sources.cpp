// ref_sources.cpp — TEST INFRASTRUCTURE ONLY.
//
// extern "C" entry points over the reference's own hand-written codec source: the Makefile compiles
// src/sbe_encoder.cpp of the reference tree where it lies (nothing is copied) together with this
// file into oracle/_ref/libsbe_ref_src.so (git-ignored), against the reference's headers and the
// stand-in json/json.h of oracle/refsrc_standin.  That pins MessageParser::parse_message with its
// dispatch, session unwrap, SessionEvent decode, Ack printable-run heuristic, error strings and
// _sequence_number lookup, the ParseResult predicates, classify_topic, SBEEncoder::
// encode_topic_message and the host-side helpers, to the reference's compiled code.
//
// Not covered: the JSON reader under the lookup is the project's own;
// src/ack_decoder.cpp does not compile against include/model/Acknowledgment.h, and
// message_handler.cpp's on_egress calls it; order_types.cpp and commit_manager.cpp need jsoncpp's
// writer.
//
// The library is built with hidden visibility and exports these entries alone: the host mirror
// defines the same C++ names in the same namespace, and both are loaded into one process.
#include <cstdint>
#include <cstring>
#include <exception>
#include <string>
#include <string_view>

#include "aeron_cluster/protocol.hpp"
#include "aeron_cluster/sbe_messages.hpp"
#include "aeron_cluster/topic_router.hpp"

#include "parse_line.hpp"

#define REFSRC_API extern "C" __attribute__((visibility("default")))

namespace {

uint64_t put(const std::string& s, uint8_t* out, uint64_t cap, uint64_t at) {
    if (at + s.size() <= cap) std::memcpy(out + at, s.data(), s.size());
    return at + s.size();
}

}  // namespace

// MessageParser::parse_message on rec[0, len).  strings: error_message, message_type, message_id,
// payload, headers back to back in sbuf, their lengths in slen[5].  nums[12]: success, timestamp,
// sequence_number (bits), template_id, schema_id, version, block_length, correlation_id,
// session_id, leader_member_id, event_code, leadership_term_id.  preds[4]: is_session_event,
// is_topic_message, is_acknowledgment, is_order_message of that result.
// Returns 0, 97 (an exception left parse_message: it never should), 98 (sbuf too small).
REFSRC_API int refsrc_parse_message(const uint8_t* rec, uint64_t len, uint8_t* sbuf, uint64_t cap, uint64_t* slen,
                                    int64_t* nums, uint8_t* preds) {
    aeron_cluster::ParseResult r;
    try {
        r = aeron_cluster::MessageParser::parse_message(rec, len);
    } catch (const std::exception&) {
        return 97;
    }
    const std::string* s[5] = {&r.error_message, &r.message_type, &r.message_id, &r.payload, &r.headers};
    uint64_t at = 0;
    for (int k = 0; k < 5; ++k) {
        slen[k] = s[k]->size();
        at = put(*s[k], sbuf, cap, at);
    }
    nums[0] = r.success ? 1 : 0;
    nums[1] = r.timestamp;
    nums[2] = (int64_t)r.sequence_number;
    nums[3] = r.template_id;
    nums[4] = r.schema_id;
    nums[5] = r.version;
    nums[6] = r.block_length;
    nums[7] = r.correlation_id;
    nums[8] = r.session_id;
    nums[9] = r.leader_member_id;
    nums[10] = r.event_code;
    nums[11] = r.leadership_term_id;
    preds[0] = r.is_session_event();
    preds[1] = r.is_topic_message();
    preds[2] = r.is_acknowledgment();
    preds[3] = r.is_order_message();
    return at <= cap ? 0 : 98;
}

// classify_topic (topic_router.hpp): 0 Unknown, 1 Orders, 2 Control (SBE_TC_*'s numbering)
REFSRC_API int refsrc_classify_topic(const uint8_t* topic, uint64_t len) {
    switch (aeron_cluster::classify_topic(std::string_view(reinterpret_cast<const char*>(topic), len))) {
        case aeron_cluster::TopicClass::Orders: return 1;
        case aeron_cluster::TopicClass::Control: return 2;
        default: return 0;
    }
}

// SBEEncoder::encode_topic_message itself.  Returns 0 and the record, 1 and the exception's text in
// err (NUL-terminated, cut to errcap), 98 when out is too small.
REFSRC_API int refsrc_encode_topic_message(const uint8_t* const* s, const uint32_t* len, int64_t ts, uint8_t* out,
                                           uint64_t cap, uint64_t* out_len, char* err, uint64_t errcap) {
    std::string f[5];
    for (int k = 0; k < 5; ++k) f[k].assign(reinterpret_cast<const char*>(s[k]), len[k]);
    *out_len = 0;
    try {
        const std::vector<uint8_t> rec = aeron_cluster::SBEEncoder::encode_topic_message(f[0], f[1], f[2], f[3], f[4], ts);
        if (rec.size() > cap) return 98;
        std::memcpy(out, rec.data(), rec.size());
        *out_len = rec.size();
        return 0;
    } catch (const std::exception& e) {
        if (errcap) {
            std::strncpy(err, e.what(), errcap - 1);
            err[errcap - 1] = '\0';
        }
        return 1;
    }
}

// The canonical line of parse_line.hpp for one record: what = 1 the ParseResult part, 2 the part
// read from the bytes alone, 4 is_acknowledgment_for; parts are joined by one blank.  Returns the
// line's length (the line is written when it fits cap).
REFSRC_API uint64_t refsrc_describe(const uint8_t* rec, uint64_t len, uint32_t what, uint8_t* out, uint64_t cap) {
    std::string line;
    auto add = [&](const std::string& part) { line += (line.empty() ? "" : " ") + part; };
    aeron_cluster::ParseResult r;
    if (what & 5) r = aeron_cluster::MessageParser::parse_message(rec, len);
    if (what & 1) add(parse_line::of_result(r));
    if (what & 2) add(parse_line::of_bytes(rec, len));
    if (what & 4) add(parse_line::of_ack_for(rec, len, r.message_id));
    put(line, out, cap, 0);
    return line.size();
}
