// aeron_cluster_amd.hpp — C++17 host mirror of the reference's codec surface, backed by the
// MI355X kernels behind include/sbecodec.h.
//
// Same names, argument meaning and error behaviour as the reference (paths relative to it):
//   SBEEncoder::encode_topic_message   include/aeron_cluster/sbe_messages.hpp:158-164,
//                                      src/sbe_encoder.cpp:131-167 (E109 → std::runtime_error)
//   MessageParser::parse_message       include/aeron_cluster/sbe_messages.hpp:422, src/sbe_encoder.cpp:513-551
//   ParseResult                        include/aeron_cluster/sbe_messages.hpp:306-412
//   decode_ack / AckInfo               include/aeron_cluster/ack_decoder.hpp:9-19, src/ack_decoder.cpp:29-105
//   MessageHandler::on_egress          include/aeron_cluster/message_handler.hpp:35-89 (E100 escapes
//                                      as std::runtime_error("buffer too short [E100]"))
//   SessionManager frame               create_topic_message + send_combined_message,
//                                      src/session_manager.cpp:936-967, :1018-1046, :1050-1144
//   CommitManager                      build_commit_offset_message (CommitOffsetLite),
//                                      src/commit_manager.cpp:16-22, :107-132; CommitOffset
//                                      include/aeron_cluster/commit_manager.hpp:17-24; commit_message /
//                                      get_last_commit / get_all_commits, src/commit_manager.cpp:29-51
//   handle_incoming_message's commit   src/cluster_client.cpp:1198-1303 (should_skip_auto_commit
//                                      :847-886, extract_topic_from_message :756-806): AutoCommitter
//   LocalFragmentReassembler           src/cluster_client.cpp:39-82 (FragmentReassembler below)
//   ClusterClient::offer_ingress       include/aeron_cluster/cluster_client.hpp:409 — the sink the
//                                      encoded records are handed to (OfferFn below)
// plus batched overloads, which are the point of the GPU path: one launch per batch.
//
// Everything computes on the GPU.  There is no CPU codec here: without a gfx950 device every
// codec entry point throws std::runtime_error("sbecodec: ...") (SBEUtils, SBEDecoder and the
// header-only MessageParser helpers are host struct readers, as in the reference).  Host work is
// staging and result building only, on min(16, cores) host threads (AERON_AMD_HOST_THREADS):
//  - a batch of at most 65536 records and 8-32 MiB (AERON_AMD_CHUNK_BYTES) is one chunk; up to
//    4 MiB staged (AERON_AMD_ZC_BYTES) it takes the zero-copy path: the kernels read the
//    page-locked staging buffer and write the results straight into the page-locked result
//    block over PCIe, one launch (encode: two) and one wait, no copy step;
//  - larger batches are cut into chunks that flow through three HIP streams (copy-in, kernels,
//    copy-out) three slots deep, so chunk k+1's H2D, chunk k's kernels and chunk k-1's D2H
//    overlap while the host threads stage the next chunk.
#pragma once

#include <cstdint>
#include <chrono>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

namespace aeron_cluster {

// include/aeron_cluster/config.hpp:169-199
namespace SBEConstants {
constexpr std::uint16_t CLUSTER_SCHEMA_ID = 111;
constexpr std::uint16_t CLUSTER_SCHEMA_VERSION = 8;
constexpr std::uint16_t TOPIC_SCHEMA_ID = 1;
constexpr std::uint16_t TOPIC_SCHEMA_VERSION = 1;
constexpr std::uint16_t SESSION_CONNECT_TEMPLATE_ID = 3;
constexpr std::uint16_t SESSION_EVENT_TEMPLATE_ID = 2;
constexpr std::uint16_t SESSION_CLOSE_TEMPLATE_ID = 4;
constexpr std::uint16_t SESSION_KEEPALIVE_TEMPLATE_ID = 5;
constexpr std::uint16_t TOPIC_MESSAGE_TEMPLATE_ID = 1;
constexpr std::uint16_t ACKNOWLEDGMENT_TEMPLATE_ID = 2;
constexpr std::uint16_t SESSION_CONNECT_BLOCK_LENGTH = 16;
constexpr std::uint16_t SESSION_EVENT_BLOCK_LENGTH = 32;
constexpr std::uint16_t TOPIC_MESSAGE_BLOCK_LENGTH = 48;
constexpr std::uint16_t ACKNOWLEDGMENT_BLOCK_LENGTH = 8;
constexpr std::int32_t SESSION_EVENT_OK = 0;
constexpr std::int32_t SESSION_EVENT_ERROR = 1;
constexpr std::int32_t SESSION_EVENT_REDIRECT = 2;
constexpr std::int32_t SESSION_EVENT_AUTHENTICATION_REJECTED = 3;
constexpr std::int32_t SESSION_EVENT_CLOSED = 4;
constexpr std::size_t SBE_HEADER_LENGTH = 8;
}  // namespace SBEConstants

// include/aeron_cluster/sbe_messages.hpp:14-20: the 8-byte SBE message header, packed
struct MessageHeader {
    std::uint16_t block_length;
    std::uint16_t template_id;
    std::uint16_t schema_id;
    std::uint16_t version;
} __attribute__((packed));
static_assert(sizeof(MessageHeader) == 8, "MessageHeader must be exactly 8 bytes");

// include/aeron_cluster/sbe_messages.hpp:39-54: SessionEvent's 32-byte fixed block (template 2,
// schema 111), packed
struct SessionEvent {
    std::int64_t correlation_id;
    std::int64_t cluster_session_id;
    std::int64_t leadership_term_id;
    std::int32_t leader_member_id;
    std::int32_t code;
    static constexpr std::uint16_t sbe_block_length() { return 32; }
    static constexpr std::uint16_t sbe_template_id() { return 2; }
    static constexpr std::uint16_t sbe_schema_id() { return 111; }
    static constexpr std::uint16_t sbe_schema_version() { return 8; }
} __attribute__((packed));
static_assert(sizeof(SessionEvent) == 32, "SessionEvent must be exactly 32 bytes");

// include/aeron_cluster/sbe_messages.hpp:189-247, bodies src/sbe_encoder.cpp:174-323: the
// reference's one-record struct readers.  Host code: each is a header / fixed-block copy plus at
// most three u32-length-prefixed strings, and none is on the batch decode path (parse_message
// reaches SessionEvent through the GPU decode, whose fields these return for the same record; the
// u32-prefixed Acknowledgment layout of decode_acknowledgment is unreachable from parse_message,
// whose is_topic_message() claims template 2 / schema 1 first, src/sbe_encoder.cpp:536-544).
// decode_topic_message is declared by the reference but never defined (no definition in src/), so
// it is not provided here either.
class SBEDecoder {
public:
    // :174-181: false for null data or fewer than 8 bytes, else the header bytes
    static bool decode_message_header(const std::uint8_t* data, std::size_t length, MessageHeader& header);
    // :183-238: false below 40 bytes or unless template 2 / schema 111; event = the 32-B block;
    // detail = the u32-prefixed string after it when one fits (<= 10 MiB; empty when its length is
    // 0; left as the caller had it when the prefix or the string does not fit)
    static bool decode_session_event(const std::uint8_t* data, std::size_t length, SessionEvent& event,
                                     std::string& detail);
    // :240-282: false below 16 bytes, unless template 2 / schema 1, or when message_id or status (u32
    // prefixes after the 8-B block) do not fit; error is read when bytes remain after status;
    // timestamp = the i64 after the header (written whenever the header checks pass)
    static bool decode_acknowledgment(const std::uint8_t* data, std::size_t length, std::string& message_id,
                                      std::string& status, std::string& error, std::int64_t& timestamp);
};

// The reference's debug helpers (include/aeron_cluster/sbe_messages.hpp:252-301, bodies
// src/sbe_encoder.cpp:328-485).  Host-side formatting only: ParseResult::get_description and the
// reference's tools (tools/message_inspector.cpp) call them; none of them is on the codec path.
namespace SBEUtils {
void print_hex_dump(const std::uint8_t* data, std::size_t length, const std::string& prefix = "",
                    std::size_t max_bytes = 0);
std::string get_session_event_code_string(std::int32_t code);           // :370-385
std::string get_message_type_name(std::uint16_t template_id, std::uint16_t schema_id);  // :387-409
bool is_valid_correlation_id(std::int64_t correlation_id);             // :411-413
std::int64_t generate_correlation_id();                                 // :415-419
std::string format_timestamp(std::int64_t timestamp);                   // :421-433
bool is_valid_sbe_message(const std::uint8_t* data, std::size_t length);  // :435-457
std::vector<std::string> extract_readable_strings(const std::uint8_t* data, std::size_t length,
                                                  std::size_t min_length = 3);  // :459-485
}  // namespace SBEUtils

// include/aeron_cluster/sbe_messages.hpp:306-328 (fields), :332-411 (predicates, description)
struct ParseResult {
    bool success = false;
    std::string error_message;
    std::string message_type;
    std::string message_id;
    std::string payload;
    std::string headers;
    std::int64_t timestamp = 0;
    std::uint64_t sequence_number = 0;
    std::uint16_t template_id = 0;
    std::uint16_t schema_id = 0;
    std::uint16_t version = 0;
    std::uint16_t block_length = 0;
    std::int64_t correlation_id = 0;
    std::int64_t session_id = 0;
    std::int32_t leader_member_id = 0;
    std::int32_t event_code = 0;
    std::int64_t leadership_term_id = 0;
    // sequence_number: "_sequence_number" of the payload JSON (src/sbe_encoder.cpp:1031-1125),
    // evaluated on the device with jsoncpp 1.9.5 semantics (sbe_eval_sequence_numbers; jsoncpp is
    // absent here, so parity with it is unpinned).  sequence_key_present: the payload holds the
    // literal key bytes (SBE_FL_SEQ_KEY).
    bool sequence_key_present = false;

    bool is_session_event() const {
        return template_id == SBEConstants::SESSION_EVENT_TEMPLATE_ID && schema_id == SBEConstants::CLUSTER_SCHEMA_ID;
    }
    bool is_topic_message() const;
    bool is_acknowledgment() const {
        return template_id == SBEConstants::ACKNOWLEDGMENT_TEMPLATE_ID && schema_id == SBEConstants::TOPIC_SCHEMA_ID;
    }
    // sbe_messages.hpp:382-406: a topic message whose type or payload names order content
    bool is_order_message() const;
    // src/sbe_encoder.cpp:490-510: "<type name>[ (code: …)| (type: …)][ [ID: <8 chars>...]]" or
    // "Parse Error: <error_message>"
    std::string get_description() const;
};

// include/aeron_cluster/ack_decoder.hpp:9-15
struct AckInfo {
    std::uint64_t timestamp_nanos{};
    std::string message_id;
    std::string topic;
    std::string correlation_id;
    bool simple_control_ack{false};
};

// One TopicMessage's fields, wire order (TopicMessage.h:515-1231).
struct TopicMessageFields {
    std::string_view topic, message_type, uuid, payload, headers;
    std::int64_t timestamp = 0;  // 0 → the encoder's clock, as the reference does
};

namespace detail {
struct HostBytesAccess;
struct Descriptors;
}  // namespace detail

// An array in page-locked host memory taken from a recycled pool: the device writes results
// straight into it (DMA, or the kernels themselves on the zero-copy path: no staging copy, no zero
// fill, no page faults on reuse), and the caller reads it in place.
// Aliasing: copying a HostArray (or an EncodedBatch) copies a reference, not the bytes: the copies
// share one block, and the arrays of one EncodedBatch (offsets, status, bytes) share one block.
// to_vector() makes an independent copy.  Retention: the block (a power of two of at least 4 KiB)
// stays page-locked while any copy lives, then returns to the pool, which keeps up to
// AERON_AMD_PINNED_CACHE_BYTES (default 4 GiB) of free blocks for reuse; a caller that holds many
// small results pins at least 4 KiB per result.
template <class T>
class HostArray {
public:
    const T* data() const { return p_; }
    T* data() { return p_; }
    std::size_t size() const { return n_; }
    bool empty() const { return n_ == 0; }
    const T* begin() const { return p_; }
    const T* end() const { return p_ + n_; }
    T* begin() { return p_; }
    T* end() { return p_ + n_; }
    const T& operator[](std::size_t i) const { return p_[i]; }
    T& operator[](std::size_t i) { return p_[i]; }
    const T& back() const { return p_[n_ - 1]; }
    std::vector<T> to_vector() const { return std::vector<T>(begin(), end()); }
    friend bool operator==(const HostArray& a, const std::vector<T>& v) {
        if (a.n_ != v.size()) return false;
        for (std::size_t i = 0; i < a.n_; ++i)
            if (!(a.p_[i] == v[i])) return false;
        return true;
    }

private:
    friend struct detail::HostBytesAccess;
    std::shared_ptr<void> block_;
    T* p_ = nullptr;
    std::size_t n_ = 0;
};
using HostBytes = HostArray<std::uint8_t>;

// A packed batch of encoded records: record i = bytes[offsets[i], offsets[i+1]).
struct EncodedBatch {
    HostBytes bytes;
    HostArray<std::uint64_t> offsets;
    HostArray<std::uint8_t> status;  // SBE_ENC_* per record
    std::string_view record(std::size_t i) const {
        return {reinterpret_cast<const char*>(bytes.data()) + offsets[i], static_cast<std::size_t>(offsets[i + 1] - offsets[i])};
    }
};

enum class EncodeLength {
    Reference,  // exactly what SBEEncoder::encode_topic_message returns (26+Σlen)
    Wire,       // the full wire record (34+Σlen), computeLength's E109 above 65534 B
    Publish     // ClusterClient::publish_topic's put*(const char*, int) calls (src/cluster_client.cpp:
                // 1850-1854): wire length, each length mod 65536 with that many bytes, no E109
};

class SBEEncoder {
public:
    // src/sbe_encoder.cpp:131-167: timestamp 0 → system_clock milliseconds; throws
    // std::runtime_error("<field>Length too long for length type [E109]") above 65534 bytes.
    static std::vector<std::uint8_t> encode_topic_message(const std::string& topic, const std::string& message_type,
                                                          const std::string& uuid, const std::string& payload,
                                                          const std::string& headers, std::int64_t timestamp = 0);
    // Batch encode: one GPU launch; records with E109 get status != 0 and zero bytes.
    static EncodedBatch encode_topic_batch(const std::vector<TopicMessageFields>& msgs,
                                           EncodeLength length = EncodeLength::Wire);
    // src/sbe_encoder.cpp:169-172: high_resolution_clock ticks since its epoch (nanoseconds)
    static std::int64_t get_current_timestamp();
};

class ParsedBatch;

// One member path of a JSON document for ParsedBatch::extract / extract_json_documents
// (sbe_json_extract_batch): 1..4 decoded member names, raw bytes.  A std::string or a literal is
// split at its dots ("message.message.order_id"); a list of names is taken as it is.
struct JsonPath {
    std::vector<std::string> names;
    JsonPath(const char* dotted) : JsonPath(std::string(dotted)) {}
    JsonPath(const std::string& dotted);
    JsonPath(std::vector<std::string> parts) : names(std::move(parts)) {}
};

// sbe_json_extract_batch's outputs on the host (include/sbecodec.h: SBE_JX_*), with views into the
// caller's bytes (valid while they are) and Value::asString's conversions.
class JsonFields {
public:
    std::size_t size() const { return doc_.size(); }
    std::size_t paths() const { return n_paths_; }
    std::uint8_t doc(std::size_t i) const { return doc_[i]; }              // SBE_JX_OK .. SBE_JX_STACK
    std::uint8_t root_kind(std::size_t i) const { return root_[i]; }
    std::uint8_t kind(std::size_t i, std::size_t p) const { return kind_[i * n_paths_ + p]; }  // SBE_JX_MISSING .. ARRAY
    // strings: the bytes between the quotes, escapes undecoded; numbers and literals: the token;
    // containers: bracket to bracket; MISSING: empty
    std::string_view token(std::size_t i, std::size_t p) const;
    bool is_string(std::size_t i, std::size_t p) const;
    // Value::asString (jsoncpp 1.9.5): the decoded string, a number as valueToString prints it,
    // "true" / "false", "" for null and for a missing member (Value::get's null); a container throws
    // std::runtime_error
    std::string as_string(std::size_t i, std::size_t p) const;
    // Value::asUInt64: null and a missing member 0, bools 0 / 1, integers in range exact, a real in
    // [0, 2^64) truncated after strtod; a negative integer, a real outside that range, a string or
    // a container throws std::runtime_error
    std::uint64_t as_uint64(std::size_t i, std::size_t p) const;

private:
    friend struct JsonExtractAccess;
    std::size_t n_paths_ = 0;
    std::vector<std::uint8_t> doc_, root_, kind_;
    std::vector<std::uint32_t> off_, len_;
    std::vector<const char*> base_;  // record i's first byte
};

// The same for bare documents (dec == NULL): document i is docs[i]; views point into docs.
JsonFields extract_json_documents(const std::vector<std::string>& docs, const std::vector<JsonPath>& paths);

// What the reference's subscriber reads out of an Order message
// (examples/pubsub_reconnect_test.cpp:576-620): message.message.client_order_id (else
// message.message.order_details.client_order_id; with a non-object message.message the older
// message.order_details.client_order_id), message.message.order_id, and the top-level uuid for an
// empty order_id; only strings count.  Records the example does not look at (neither
// is_order_message() nor a CREATE_ORDER topic message), an empty payload, a parse failure and
// everything that throws there (a root that is neither an object nor null, the stack limit) give
// two empty strings, as its catch (...) does.
struct OrderIds {
    std::string client_order_id, order_id;
};
std::vector<OrderIds> extract_order_ids(const ParsedBatch& batch);
OrderIds extract_order_ids(const ParseResult& result);

// include/aeron_cluster/topic_router.hpp: "orders" and "order_request_topic" are Orders;
// "_subscriptions", "_ack", "_control" and "_internal" are Control.
enum class TopicClass { Orders, Control, Unknown };
TopicClass classify_topic(std::string_view topic);

// ParsedBatch::order_select's result (sbe_order_select): what the ParseResult predicates say of
// every record, without building a ParseResult.
class MessageKinds {
public:
    std::size_t size() const { return pred_.size(); }
    // SBE_PR_* bits: result(i).is_session_event() / is_topic_message() / is_acknowledgment() / is_order_message()
    std::uint8_t pred(std::size_t i) const { return pred_[i]; }
    // the subscriber's test (examples/pubsub_reconnect_test.cpp:578-579) on a TopicMessage record
    bool selected(std::size_t i) const { return select_[i] != 0; }
    TopicClass topic_class(std::size_t i) const;  // classify_topic of a TopicMessage's topic; Unknown for other records
    std::uint64_t selected_count() const { return totals_[0]; }
    std::uint64_t order_count() const { return totals_[1]; }  // records with is_order_message()

private:
    friend class ParsedBatch;
    std::vector<std::uint8_t> pred_, select_, class_;
    std::uint64_t totals_[2] = {0, 0};
};

class MessageParser {
public:
    // src/sbe_encoder.cpp:513-551 (never throws; success = false + error_message)
    static ParseResult parse_message(const std::uint8_t* data, std::size_t length);
    // src/sbe_encoder.cpp:957-1143 called directly (sbe_messages.hpp:423): no dispatch — a header
    // other than template 1 / schema 1 gives "Not a TopicMessage (got template_id=T, schema_id=S)",
    // fewer than 8 bytes the flyweight's E107 ("SBE TopicMessage decoding failed: buffer too short
    // for flyweight [E107]"); otherwise the GPU decode of the record.
    static ParseResult decode_topic_message_with_sbe(const std::uint8_t* data, std::size_t length);
    // src/sbe_encoder.cpp:833-954 called directly (sbe_messages.hpp:424): the printable-run
    // heuristic on any record whose header says template 2 / schema 1.
    static ParseResult decode_acknowledgment_with_sbe(const std::uint8_t* data, std::size_t length);
    // src/sbe_encoder.cpp:554-575: parse_message plus the reference's diagnostics (hex dump of
    // records of 1..200 bytes on stdout; DEBUG_LOG lines when AERON_CLUSTER_DEBUG=1).
    static ParseResult parse_message_debug(const std::uint8_t* data, std::size_t length,
                                           const std::string& debug_prefix = "");
    // src/sbe_encoder.cpp:577-586: "INVALID" below 8 bytes, else the header's type name
    static std::string get_message_type(const std::uint8_t* data, std::size_t length);
    // src/sbe_encoder.cpp:588-603: the i64 after the header of a schema-111 message, else 0
    static std::int64_t extract_correlation_id(const std::uint8_t* data, std::size_t length);
    // src/sbe_encoder.cpp:605-616
    static bool is_acknowledgment_for(const std::uint8_t* data, std::size_t length, const std::string& message_id);

    // Batch: records data[rec_off[i], rec_off[i+1]), ParseResults built on the host threads.
    static std::vector<ParseResult> parse_batch(const std::uint8_t* data, const std::uint64_t* rec_off, std::size_t n);
    // The same into the caller's vector (resized to n): each ParseResult is rewritten in place and
    // keeps its string buffers, so a caller that parses batch after batch into one vector does not
    // allocate once the strings have grown (out[i] == parse_message(record i) either way).
    static void parse_batch(const std::uint8_t* data, const std::uint64_t* rec_off, std::size_t n,
                            std::vector<ParseResult>& out);
    // Batch without materialising: the device descriptors and views into `data` (valid while the
    // caller's bytes are), ParseResults built on demand.  See ParsedBatch.
    static ParsedBatch decode_batch(const std::uint8_t* data, const std::uint64_t* rec_off, std::size_t n);
};

// parse_message's outcome for a batch, kept as the device descriptors (host copy) plus views into
// the caller's records.  result(i) == MessageParser::parse_message(record i); the string_view
// accessors give the same bytes without building the ParseResult.
class ParsedBatch {
public:
    std::size_t size() const { return n_; }
    ParseResult result(std::size_t i) const;
    ParseResult operator[](std::size_t i) const { return result(i); }
    // result(i) written into `out`, which keeps its string buffers (no allocation once they have grown)
    void result_into(std::size_t i, ParseResult& out) const;
    bool success(std::size_t i) const;
    std::uint8_t status(std::size_t i) const;  // SBE_ST_* of include/sbecodec.h
    std::uint16_t template_id(std::size_t i) const;
    std::uint16_t schema_id(std::size_t i) const;
    std::int64_t timestamp(std::size_t i) const;
    std::uint64_t sequence_number(std::size_t i) const;
    // TopicMessage: message_type / message_id (uuid) / payload / headers views; other statuses:
    // the views ParseResult would copy (Ack defaults and error texts are not views: use result(i)).
    std::string_view view(std::size_t i, int field) const;
    // Calls fn(i, result(i)) in record order on the calling thread; the ParseResults of each
    // 4096-record block are built on the host threads first.
    void for_each(const std::function<void(std::size_t, const ParseResult&)>& fn) const;
    // The JSON members at `paths` of every TopicMessage's payload (view 3) or headers (view 4), read
    // on the device as Json::parseFromStream with builder defaults reads them
    // (sbe_json_extract_batch); select: null, or n bytes, 0 skips the record.
    JsonFields extract(const std::vector<JsonPath>& paths, int view = 3, const std::uint8_t* select = nullptr) const;
    // The ParseResult predicates of every record, the subscriber's order test and the topic class,
    // computed on the device from the descriptors and the record bytes (sbe_order_select).
    MessageKinds order_select() const;

private:
    friend class MessageParser;
    friend struct JsonExtractAccess;
    friend class AutoCommitter;
    friend class DeliveryTracker;
    std::shared_ptr<const detail::Descriptors> desc_;  // host copy of the device descriptors
    const std::uint8_t* data_ = nullptr;               // the caller's records (borrowed)
    const std::uint64_t* rec_off_ = nullptr;           // the caller's offsets (borrowed)
    std::size_t n_ = 0;
};

std::optional<AckInfo> decode_ack(const std::uint8_t* data, std::size_t len);

// MessageParser::parse_message at the reference's call granularity, batched across polls.  The
// reference parses one fragment per call from its poll handler (handle_incoming_message,
// src/cluster_client.cpp:1185) in polls of up to 100 fragments
// (include/aeron_cluster/performance_config.hpp:17); one GPU call per fragment costs a launch or
// a serve round trip, far more than the parse.  A BatchingParser takes the fragments of many
// polls: on_fragment copies each one (the fragment is only valid during the poll callback) into
// a page-locked batch; when the batch holds max_records records or max_bytes bytes, or at a poll()
// whose oldest pending record has waited max_delay, the batch goes to a decode thread
// (MessageParser::decode_batch) and filling continues in another batch (`batches` are kept; more
// are made when the caller hands off faster than it polls).  Handlers run on the caller's thread,
// in arrival order, only inside poll() / flush(), with handler(result) ==
// handler(MessageParser::parse_message(fragment)); on_fragment never runs a handler.  Waits spin
// for `spin` before they block.  A handler that throws propagates out of poll() / flush(); the
// records after it are delivered by the next call, none twice.  Call poll() after every poll of
// the subscription (the reference's loop), or flush().
// Added latency per record: at most max_delay + one batch decode after the poll that follows it
// (a caller polling continuously), or whatever the caller waits between polls.
class BatchingParser {
public:
    struct Options {
        std::size_t max_records = 8192;
        std::size_t max_bytes = std::size_t(4) << 20;
        std::chrono::microseconds max_delay{200};
        std::size_t batches = 4;               // batches kept (2..64)
        std::chrono::microseconds spin{200};   // spin before blocking in a wait (0: block at once)
    };
    using Handler = std::function<void(const ParseResult&)>;
    explicit BatchingParser(Handler handler);
    BatchingParser(Handler handler, Options options);
    ~BatchingParser();  // flush(): every record given is delivered
    BatchingParser(const BatchingParser&) = delete;
    BatchingParser& operator=(const BatchingParser&) = delete;

    void on_fragment(const std::uint8_t* data, std::size_t length);
    // After each poll: delivers every decoded batch; hands the filling batch to the decoder if its
    // oldest record has waited max_delay.  Returns the records delivered.
    std::size_t poll();
    // Decodes everything given so far and delivers it.  Returns the records delivered.
    std::size_t flush();
    std::size_t pending() const;  // given but not yet delivered
    std::uint64_t delivered() const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

using TopicMessageCallback = std::function<void(std::string_view topic, std::string_view msg_type,
                                                std::string_view uuid, std::string_view payload,
                                                std::string_view headers)>;
using AckCallback = std::function<void(const AckInfo&)>;

class MessageHandler {
public:
    MessageHandler();
    ~MessageHandler();
    void handleMessage(const ParseResult& result);  // src/message_handler.cpp:10-16
    void on_egress(const std::uint8_t* data, std::size_t len);
    // Batch form: callbacks in record order; a record where the reference throws stops the batch
    // with the same std::runtime_error after the callbacks of the records before it.
    void on_egress_batch(const std::uint8_t* data, const std::uint64_t* rec_off, std::size_t n);
    void set_topic_message_callback(TopicMessageCallback cb) { tm_cb_ = std::move(cb); }
    void set_ack_callback(AckCallback cb) { ack_cb_ = std::move(cb); }

private:
    TopicMessageCallback tm_cb_;
    AckCallback ack_cb_;
};

// The frame SessionManager::Impl publishes (src/session_manager.cpp:1050-1144): the 32-B
// SessionMessageHeader {24, 1, 111, 8, leadershipTermId, clusterSessionId, 0} followed by
// create_topic_message's record (26+Σlen bytes, timestamp = high_resolution_clock nanoseconds).
class SessionFrameEncoder {
public:
    // update_session_header (:1018-1046)
    void update_session_header(std::int64_t leadership_term_id, std::int64_t cluster_session_id) {
        leadership_term_id_ = leadership_term_id;
        cluster_session_id_ = cluster_session_id;
    }
    // One frame as send_combined_message builds it (:1118-1144); throws E109 like
    // create_topic_message (:1111-1114).
    std::vector<std::uint8_t> create_combined_message(const std::string& topic, const std::string& message_type,
                                                      const std::string& message_id, const std::string& payload,
                                                      const std::string& headers) const;
    // Batch: one GPU launch.  A message's timestamp 0 → the nanosecond clock.
    EncodedBatch encode_batch(const std::vector<TopicMessageFields>& msgs,
                              EncodeLength length = EncodeLength::Reference) const;

private:
    std::int64_t leadership_term_id_ = 0, cluster_session_id_ = 0;
};

// The raw ingress sink (ClusterClient::offer_ingress signature, include/aeron_cluster/cluster_client.hpp:409).
using OfferFn = std::function<bool(const std::uint8_t* data, std::size_t len)>;

// What ClusterClient::on_ack_default (src/cluster_client.cpp:1924-1941) computes for one ack:
// matched: message_id was in flight (the entry is erased), rtt_ns = (int64)now - (int64)send_ns;
// otherwise rtt_ns = (int64)now - (int64)ack.timestamp_nanos, the reference's est_rtt.
struct AckMatch {
    bool matched = false;
    std::int64_t rtt_ns = 0;
};

// ClusterClient's inflight_ (include/aeron_cluster/cluster_client.hpp:420) with remember_outgoing
// (src/cluster_client.cpp:1920-1922) and on_ack_default (:1924-1941).  State: one device table
// (sbe_inflight_*, keys up to SBE_INFLIGHT_KEY_MAX = 40 bytes) and a host std::unordered_map for
// longer keys; a key goes to one or the other by its length, decided on the host, so no status is
// read back after a remember.  Before a batch that would take the table's used slots past half
// its capacity, the table is rehashed into one with room (erased slots are reclaimed; the capacity
// doubles as often as needed).
// Cost: every call copies its keys / records to the device and waits for the result on a stream of
// its own.  The single forms (remember_outgoing, on_ack) are one-record batches: two launches plus
// the copies, tens of microseconds where the reference's map needs well under one; use them for
// compatibility and the batch forms for throughput.  on_egress_batch decodes the records on the
// device (sbe_decode_batch, SBE_DEC_ON_EGRESS) and matches the descriptors where they lie: only
// a code and a time per record come back.  One thread at a time.
class AckCorrelator {
public:
    explicit AckCorrelator(std::uint64_t initial_capacity = 1u << 16, std::uint32_t tag_bits = 0);
    ~AckCorrelator();
    AckCorrelator(const AckCorrelator&) = delete;
    AckCorrelator& operator=(const AckCorrelator&) = delete;

    void remember_outgoing(const std::string& uuid, std::uint64_t ts_nanos);
    // remember_outgoing(uuids[i], ts[i]) for every i, in order (ts.size() == uuids.size())
    void remember_batch(const std::vector<std::string>& uuids, const std::vector<std::uint64_t>& ts_nanos);
    AckMatch on_ack(const AckInfo& ack, std::uint64_t now_ns);
    // MessageHandler::on_egress over the records with on_ack_default as its ack callback: one entry
    // per ack (simple or full), in record order; other records give none.
    std::vector<AckMatch> on_egress_batch(const std::uint8_t* data, const std::uint64_t* rec_off, std::size_t n,
                                          std::uint64_t now_ns);
    // entries that can still match (reads the table's header back), table capacity, rehashes so far
    std::size_t size() const;
    std::uint64_t capacity() const;
    std::uint64_t rehashes() const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// What the subscriber's callback of examples/pubsub_reconnect_test.cpp (:576-716) finds out about
// one delivered record.
struct Delivery {
    bool selected = false;            // the callback's outer if (:578) holds; false: nothing else is set
    bool already_processed = false;   // message_id was in received_message_ids (:625-635)
    std::uint32_t redeliveries = 0;   // batch form: the id's redeliveries recorded after the whole batch, i.e. what
                                      // record_duplicate_delivery (:83-90) returned for its last redelivery in it
    std::string client_order_id, order_id;  // extract_order_ids of the record
    bool duplicate_client_order = false;    // a first delivery whose client_order_id was received before (:653-661)
    bool was_sent = false;                  // client_order_id is in sent_client_order_ids (:674)
    bool latency_recorded = false;          // the first delivery that finds a send time (:680-691)
    std::int64_t latency_ns = 0;            // now_ns - send time, when latency_recorded
};

// The first ids of one of the example's reports, in std::set<std::string> order, and how many
// there are in all (printMessageComparison :130-204 prints ten and "... and N more").
struct IdEntry {
    std::string id;
    std::uint64_t value = 0;  // missing_ids: the send time; extra_ids: the id's deliveries (0 for an id over
                              // SBE_INFLIGHT_KEY_MAX bytes); redelivered_ids: its redeliveries, as
                              // duplicate_delivery_counts (:83-90) holds them
};
struct IdList {
    std::size_t total = 0;
    std::vector<IdEntry> first;
};

// printLatencyReport (:276-353) over the latencies the tracker recorded.
struct LatencyRow {
    std::int64_t latency = 0;  // in units of unit_ns
    std::uint64_t tag = 0;     // (ordinal of the on_batch / on_message call among those that reached the
                               // tables: a non-empty batch, a selected message) << 32 | record index in it
};
struct LatencyReport {
    std::uint64_t count = 0;
    std::int64_t sum = 0, min = 0, max = 0;  // sum mod 2^64; all 0 without samples
    double avg = 0.0;                        // (double)sum / (double)count, :334
    std::vector<std::int64_t> percentiles;   // one per requested pct, by the example's rank (:322-326)
    std::vector<LatencyRow> rows;            // on request: every sample, slowest first (:304)
};

// The tables that callback keeps across calls, on the device: received_message_ids with the
// per-id counts of duplicate_delivery_counts, received_client_order_ids, and the publisher's
// sent_client_order_ids / client_order_send_time (:455-459, :498-501), three sbe_inflight_* tables
// driven by sbe_inflight_note_keys / sbe_inflight_lookup_keys.  on_batch stages the batch once and
// runs extract (the nine order-id paths), sbe_delivery_keys, note (message ids), note (client
// ids) and lookup (sent) back to back on one stream; per-record codes come back, the id strings
// are cut from the caller's bytes.  Ids over SBE_INFLIGHT_KEY_MAX bytes live in host sets, ids
// spelled with escapes are decoded on the host and appended behind the staged batch before the
// table calls, so "ab\u0063" is abc.  Tables are rehashed before a batch that would take their
// used slots past half the capacity.  A batch takes one clock reading (now_ns), as
// AckCorrelator::on_egress_batch does.  Differences from the example, both in note_sent: a
// client_order_id sent twice keeps its first send time (the example overwrites it), and ids are
// expected to be noted as sent before their deliveries arrive (the publisher does, :455-501).
// One thread at a time.
class DeliveryTracker {
public:
    explicit DeliveryTracker(std::uint64_t initial_capacity = 1u << 16, std::uint32_t tag_bits = 0);
    ~DeliveryTracker();
    DeliveryTracker(const DeliveryTracker&) = delete;
    DeliveryTracker& operator=(const DeliveryTracker&) = delete;

    // the publisher's two inserts for every id
    void note_sent(const std::vector<std::string>& client_order_ids, std::uint64_t ts_ns);
    // the callback for every record of the batch, in order
    std::vector<Delivery> on_batch(const ParsedBatch& batch, std::uint64_t now_ns);
    // the one-record form: a one-record batch of keys (two launches per table, tens of microseconds)
    Delivery on_message(const ParseResult& result, std::uint64_t now_ns);
    std::uint64_t messages_received() const;  // records that were not already processed (:636-638)
    // printMessageComparison (:130-190) as counts: ids sent, ids received, sent and never answered
    // by a delivery, received and never sent
    std::size_t sent() const;
    std::size_t received() const;
    std::size_t missing() const;
    std::size_t extra() const;
    void clear_duplicate_tracking();  // :70-73: the redelivery counts start again
    std::uint64_t rehashes() const;
    // The reports the example prints from these sets, read on the device (sbe_inflight_list_keys,
    // sbe_latency_report) without copying a table back.  Each list holds the first `limit` ids
    // (at most SBE_LIST_MAX = 64; std::invalid_argument beyond) in std::string order and the
    // number of all of them; ids over SBE_INFLIGHT_KEY_MAX bytes are merged in from the host sets.
    IdList missing_ids(std::size_t limit = 10) const;      // sent and never received (:153-157)
    IdList extra_ids(std::size_t limit = 10) const;        // received and never sent (:158-162)
    IdList redelivered_ids(std::size_t limit = 10) const;  // message ids delivered more than once (:83-90)
    // Every latency on_batch / on_message recorded goes to a log on the device, in nanoseconds,
    // right behind the lookup that found it; the log grows as the tables do.  The report divides
    // by unit_ns as duration_cast does (truncation toward zero; 1 .. 2^62, 1000000: the example's
    // milliseconds): min, max and the percentiles are the divided entries of the sorted
    // nanoseconds, which is what sorting the divided samples gives; the sum of divided samples is
    // taken on the host from the sorted copy when unit_ns != 1.  pcts: at most 16 values in
    // [0, 100].  want_rows: every sample slowest first; equal latencies by descending nanoseconds,
    // then later records first.
    LatencyReport latency_report(const std::vector<double>& pcts = {75.0, 80.0, 90.0, 95.0, 99.0, 99.9, 99.99},
                                 std::uint64_t unit_ns = 1000000, bool want_rows = false) const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// ClusterClient::publish_topic (src/cluster_client.cpp:1809-1864) minus the connection checks:
// uuid = "pub_" + now_nanos() (:1818), headers "{}" when empty (:1821), timestamp now_nanos()
// (:1845), sequenceNumber 0, the put*(const char*, int) length wrap (EncodeLength::Publish), and
// the record handed to the offer_ingress-shaped sink (:1860).  Returns the uuid, as the reference
// does whether or not the offer succeeded.
class TopicPublisher {
public:
    explicit TopicPublisher(OfferFn offer) : offer_(std::move(offer)) {}
    std::string publish_topic(std::string_view topic, std::string_view message_type, std::string_view json_payload,
                              std::string_view headers_json);
    // Batch form: one GPU launch for all records, offered in order; each message gets its own uuid
    // and timestamp (msgs[i].uuid / .timestamp are ignored).  Returns the uuids.
    std::vector<std::string> publish_topic_batch(const std::vector<TopicMessageFields>& msgs);
    // With a correlator set, every record whose offer returned true is remembered with its uuid and
    // timestamp (src/cluster_client.cpp:1860-1861), one remember_batch per publish call; nullptr
    // (the default): nothing is remembered.  The correlator must outlive the publisher's calls.
    void set_correlator(AckCorrelator* correlator) { correlator_ = correlator; }

private:
    OfferFn offer_;
    AckCorrelator* correlator_ = nullptr;
};

// include/aeron_cluster/commit_manager.hpp:17-24
struct CommitOffset {
    std::string topic;
    std::string message_identifier;
    std::string message_id;
    std::uint64_t timestamp_nanos = 0;
    std::uint64_t sequence_number = 0;
};

class CommitManager {
public:
    // src/commit_manager.cpp:16-22
    static std::uint32_t topic_to_id(const std::string& topic);
    // src/commit_manager.cpp:107-132: a known topic → CommitOffsetLite (template 301) with topicId,
    // sequence, messageId, messageIdentifier; E109 → std::runtime_error.  For an unknown topic
    // (topic_to_id 0) this call still throws, as it always has: build_commit_offset_fallback builds
    // the reference's frame for it.
    std::vector<std::uint8_t> build_commit_offset_message(const std::string& topic, const std::string& client_id,
                                                          const CommitOffset& offset) const;
    // src/commit_manager.cpp:197-209: the jsoncpp text of an offset, indentation "" (keys sorted, no
    // white space): {"action":"COMMIT_OFFSET","messageIdentifier":..,"message_id":..,
    // "sequence_number":..,"timestamp_nanos":..,"topic":..}.  Host-only code, as Order::validate.
    static std::string serialize_commit_offset(const CommitOffset& offset);
    // src/commit_manager.cpp:177-195: topic, message_identifier and message_id through asString,
    // timestamp_nanos and sequence_number through asUInt64, absent members "" / 0; the document is
    // read on the device (five root paths of sbe_json_extract_batch).  A parse failure throws
    // std::runtime_error whose text begins "Failed to parse commit offset JSON: " (jsoncpp's
    // formatted error list behind the prefix is not reproduced); a root that is neither an object
    // nor null, and a member asString / asUInt64 cannot convert, throw std::runtime_error too.
    static CommitOffset parse_commit_offset(const std::string& payload);
    // One launch for all: with `errors` a document that throws leaves a default CommitOffset and
    // its message in (*errors)[i] ("" for the others); without, the first such document throws.
    static std::vector<CommitOffset> parse_commit_offsets_batch(const std::vector<std::string>& payloads,
                                                                std::vector<std::string>* errors = nullptr);
    // src/commit_manager.cpp:134-175, the unknown-topic branch of build_commit_offset_message on
    // the host, without a GPU: the TopicMessage {16,1,1,1} on "_subscriptions" of type
    // "COMMIT_OFFSET" with uuid "commit_offset_" + client_id + "_" + clock() and the text above as
    // payload, headers "{}".  Both of the reference's length quirks are kept: uuid and payload hold
    // their length mod 65536 and that many leading bytes (the std::uint16_t overloads), and a
    // record of more than 1040 bytes throws std::runtime_error("buffer too short [E100]") (the
    // 1048-byte buffer wrapped at 8).  The clock (default: the system's nanoseconds) is read twice,
    // first for the timestamp, then for the uuid, as the reference reads it.
    using ClockFn = std::function<std::uint64_t()>;
    std::vector<std::uint8_t> build_commit_offset_fallback(const std::string& client_id, const CommitOffset& offset,
                                                           const ClockFn& clock = {}) const;
    // Batch (one GPU launch); every offset's topic must be known.
    EncodedBatch build_commit_offset_batch(const std::vector<CommitOffset>& offsets) const;
    // src/commit_manager.cpp:29-35: the last commit per "topic:message_identifier"
    void commit_message(const std::string& topic, const std::string& message_identifier, const std::string& message_id,
                        std::uint64_t timestamp_nanos, std::uint64_t sequence_number);
    // src/commit_manager.cpp:37-46 (nullptr when there is none) and :48-51
    std::shared_ptr<CommitOffset> get_last_commit(const std::string& topic, const std::string& message_identifier) const;
    std::unordered_map<std::string, CommitOffset> get_all_commits() const;

private:
    mutable std::mutex commits_mutex_;
    std::unordered_map<std::string, CommitOffset> commits_;
};

// sbe_classify_commits' outputs on the host (include/sbecodec.h: SBE_CM_*, SBE_TOPIC_*).
struct CommitPlan {
    std::vector<std::uint8_t> cm, topic_src, topic_kind;
    std::vector<std::uint32_t> topic_off, topic_len, topic_idx;
    std::vector<std::uint64_t> last, count;  // per table entry; count: + unknown, + host-resolved
    std::vector<std::string> table;          // the topic table the plan was made with (entry 0: fallback)
};

// AutoCommitter::commit_and_send_batch: the session ids of the frames' SessionMessageHeader
// (send_combined_message, src/cluster_client.cpp:678-682), and what it did.
struct CommitSendOptions {
    std::int64_t leadership_term_id = 0;
    std::int64_t cluster_session_id = 0;
    bool session_frame = true;  // false: the bare CommitOffsetLite records
    bool last_only = false;     // one frame per topic-table entry (SBE_CE_LAST_ONLY)
    // Send the reference's JSON TopicMessage (src/commit_manager.cpp:134-175) for topics without a
    // numeric id instead of reporting them `unsent`.  The call reads `clock` (default: the system's
    // nanoseconds) twice: every JSON frame carries the first reading as its timestamp, and record
    // i's uuid ends in the second reading + i (sbe_emit_commit_offsets_ex's convention; the
    // reference reads the clock per record).
    bool json_fallback = false;
    std::function<std::uint64_t()> clock;
};
struct CommitSendResult {
    std::size_t commits = 0;            // commit_message calls made (commit_batch's return value)
    std::size_t offered = 0;            // frames handed to the sink
    std::size_t accepted = 0;           // of those, the ones the sink returned true for
    std::vector<std::size_t> unsent;    // committed records whose topic has id 0, ascending
    std::vector<std::size_t> too_long;  // committed records whose message_id exceeds 65534 bytes
    std::vector<std::size_t> fallback_e100;  // json_fallback: records whose JSON record exceeds 1040 bytes
                                             // (the reference throws "buffer too short [E100]")
};

// The commit branch of ClusterClient::handle_incoming_message (src/cluster_client.cpp:1251-1288)
// for a whole ParsedBatch: which records commit, and under which topic, is decided on the device
// (sbe_classify_commits: should_skip_auto_commit :847-886 and extract_topic_from_message :756-806
// per record); the host then calls CommitManager::commit_message.  The reference keeps only the
// last commit per "topic:identifier", so without a callback mask commit_batch commits once per
// topic-table entry (its last committable record) and walks only the records whose topic is not
// in the table (SBE_TOPIC_UNKNOWN) or is not a string (SBE_TOPIC_HOST: Value::asString on the
// host), all in record order; with a mask (callback_ok[i]: the message callback of record i
// succeeded, :1224-1239) it walks every committable record.  Either way the CommitManager ends up
// as after the reference's sequence, record by record (commit_record_by_record).  The dedup set
// (processed_messages_) is the caller's: it does not decide whether a record commits (:1237-1255).
// The topic table is the fallback topic (*subscribed_topics_.begin(), or "default": the caller's,
// since the reference's set is unordered) followed by the topics that have a stored identifier.
class AutoCommitter {
public:
    explicit AutoCommitter(std::string client_id, std::string fallback_topic = "default");
    // subscription_message_identifiers_[topic] = identifier (at most 63 topics, 4096 bytes in all
    // with the fallback topic: std::length_error beyond that)
    void set_message_identifier(const std::string& topic, const std::string& identifier);
    // :1264-1278: the stored identifier of the topic, else client_id
    const std::string& message_identifier(const std::string& topic) const;
    // One device launch over the batch's records and descriptors.
    CommitPlan classify(const ParsedBatch& batch) const;
    // The topic text of record i (Value::asString of the token; the fallback topic for FALLBACK).
    std::string topic(const ParsedBatch& batch, const CommitPlan& plan, std::size_t i) const;
    // Commits the batch into `commits`; returns the commit_message calls made.
    std::size_t commit_batch(const ParsedBatch& batch, CommitManager& commits,
                             const std::vector<bool>* callback_ok = nullptr) const;
    std::size_t commit_batch(const ParsedBatch& batch, const CommitPlan& plan, CommitManager& commits,
                             const std::vector<bool>* callback_ok = nullptr) const;
    // The reference's sequence: every committable record, in order.
    std::size_t commit_record_by_record(const ParsedBatch& batch, const CommitPlan& plan, CommitManager& commits,
                                        const std::vector<bool>* callback_ok = nullptr) const;
    // Both halves of ClusterClient::commit_message (src/cluster_client.cpp:626-633) for the batch:
    // the commits go into `commits` exactly as commit_batch makes them, and for every committed
    // record the frame send_commit_offset sends (:1264-1278, a CommitOffsetLite behind the session
    // header) goes to `offer`, in record order.  One staged upload; sbe_classify_commits and
    // sbe_emit_commit_offsets run back to back on the stream (the plan stays on the device between
    // them); the plan and the emit result come back in one download, the frames, whose size the
    // emit result gives, in the copy after it.  A record whose topic the device table does not
    // resolve (SBE_CE_HOST) is resolved here: with a non-zero topic_to_id its frame is built by
    // build_commit_offset_message and offered at its place; with topic id 0 its index goes to
    // `unsent`, and nothing throws.  A message_id over 65534 bytes (the reference throws E109) goes
    // to `too_long`.
    // options.json_fallback: the emit call is sbe_emit_commit_offsets_ex with a fallback, so the
    // device also builds the JSON frame of every id-0 table entry and of every plain string topic
    // outside the table (identifier: client_id), offered at their place in record order; the
    // records still left to the host (escaped or non-string topics) with id 0 get the same frame
    // from build_commit_offset_fallback.  `unsent` is then always empty; records whose frame the
    // reference could not build go to `fallback_e100`.  std::length_error when client_id exceeds
    // 4096 bytes.
    // last_only: only the last committable record of every table entry is sent (what commit_batch
    // commits without a mask); std::invalid_argument together with callback_ok.
    // std::length_error when the identifiers of the table exceed 4096 bytes.
    CommitSendResult commit_and_send_batch(const ParsedBatch& batch, CommitManager& commits, const OfferFn& offer,
                                           const CommitSendOptions& options = {},
                                           const std::vector<bool>* callback_ok = nullptr) const;

private:
    struct EmitRequest;
    // classify(), and with `emit` the emit call behind it on the same staged inputs
    CommitPlan run(const ParsedBatch& batch, EmitRequest* emit) const;
    std::string client_id_, fallback_;
    std::map<std::string, std::string> identifiers_;
};

// A decoded Lite record (CommitOffsetLite / OrderRequestLite / OrderNotificationLite flyweights).
struct LiteRecord {
    std::uint16_t template_id = 0;
    std::uint32_t topic_id = 0;
    std::uint64_t sequence = 0;
    std::vector<std::string> fields;  // var strings in wire order (2 or 3)
};
// Decoded with the generated flyweights' semantics; nullopt when the record is not a Lite
// template or a bounds check throws E100.
std::optional<LiteRecord> decode_lite(const std::uint8_t* data, std::size_t len);

// LocalFragmentReassembler (src/cluster_client.cpp:39-82) for batches of Aeron fragments: fragment
// i is data[frag_off[i], frag_off[i+1]) with header flags[i] (BEGIN 0x80, END 0x40).  Returns the
// delivered messages in order; a message whose END has not arrived yet is kept for the next call,
// exactly as the reference's accumulator.
//
// A raw block of a term buffer (whole frames with their 32-byte Aeron data-frame headers, as an
// image's block or raw poll hands them, or a host_register'ed term buffer read in place) is framed
// first: term_walk is the poll's loop over the headers on one host thread (the frame layer is
// third-party Aeron, restated from the data-frame layout, see sbe_term_scan in sbecodec.h), and
// on_term_block runs the same walk (sbe_term_scan) and the reassembly on the device.  block, len
// and start are multiples of 32 (std::invalid_argument otherwise).
struct TermFragments {
    std::vector<std::uint64_t> frag_off;  // [fragments + 1] offsets of the payloads laid back to back
    std::vector<std::uint8_t> flags;      // header byte 5 of each delivered frame
    std::vector<std::uint32_t> frag_src;  // offset of each delivered frame's header in the block
    std::uint64_t next = 0;               // the offset the walk stopped at
    std::uint32_t stop = 0;               // SBE_TERM_STOP_*
};
TermFragments term_walk(const std::uint8_t* block, std::size_t len, std::size_t start, std::size_t limit);

class FragmentReassembler {
public:
    EncodedBatch on_fragments(const std::uint8_t* data, const std::uint64_t* frag_off, const std::uint8_t* flags,
                              std::size_t n);
    // The fragments of block[start, len), at most `limit` of them, reassembled; *next: where the
    // walk stopped (the start of the next call).  The carry is kept exactly as on_fragments keeps it.
    EncodedBatch on_term_block(const std::uint8_t* block, std::size_t len, std::size_t start, std::size_t limit,
                               std::size_t* next = nullptr);
    // The same result, *next and kept carry as on_term_block for every input, through the one call
    // sbe_term_poll: the block goes to the device once and unshifted, the accumulator goes up as the
    // call's carry, and the host waits once for the six counts before the downloads (on_term_block
    // waits for the scan's counts, the reassembly's counts and the offsets one after another).
    // std::invalid_argument also when block[start, len) exceeds 2^30 bytes or, with the accumulator,
    // 2^31.
    EncodedBatch poll_term_block(const std::uint8_t* block, std::size_t len, std::size_t start, std::size_t limit,
                                 std::size_t* next = nullptr);
    std::size_t pending_bytes() const { return acc_.size(); }

private:
    std::vector<std::uint8_t> acc_;
};

// The publish side of the same frame layer: a batch of encoded records appended to a raw block of a
// term buffer with Aeron's framing (one BEGIN|END data frame a record, or BEGIN / middle / END frames
// at the MTU, the padding frame where the term ends), as ExclusivePublication::offer would one
// record at a time.  Third-party Aeron again, restated and not pinned to a source: the semantics
// are stated at sbe_term_append in sbecodec.h.  term_append is that loop on one host thread (the
// role term_walk plays for the scan); TermAppender::append_batch runs sbe_term_append on the device
// and copies the bytes it wrote, block[start, tail) and a padding header, back into `block`.  Both
// throw std::invalid_argument where sbe_term_append returns SBE_EINVAL: len or start not a
// multiple of 32, start > len, len > 2^30, mtu not a multiple of 32 in [64, 65504],
// max_message_length > 2^30.  This is a batch into a block nobody else writes, not a concurrent
// publication: there is no ordering between the frames.
struct TermHeader {
    std::int32_t session_id = 0;
    std::int32_t stream_id = 0;
    std::int32_t term_id = 0;
    std::int32_t term_offset_base = 0;  // the term offset of block[0] (the block may be a part of a term)
    std::uint8_t version = 0;
};
struct TermAppendOptions {
    static constexpr std::uint64_t kAeronRule = ~0ull;
    std::uint32_t mtu = 1408;
    std::uint64_t limit = ~0ull;                     // a record is refused once the tail is at or behind it
    std::uint64_t max_message_length = kAeronRule;   // kAeronRule: min(term_length / 8, 16 MiB)
    std::uint64_t term_length = 0;                   // 0: the block is the whole term
    TermHeader header;
    std::uint64_t effective_max_message_length(std::size_t block_len) const {
        if (max_message_length != kAeronRule) return max_message_length;
        const std::uint64_t term = term_length ? term_length : block_len, cap = 16ull << 20;
        return term / 8 < cap ? term / 8 : cap;
    }
    // throws std::invalid_argument
    void check(std::size_t len, std::size_t start) const {
        if ((len & 31) || (start & 31) || start > len) throw std::invalid_argument("term_append: block and start are multiples of 32");
        if (len > ((std::size_t)1 << 30)) throw std::invalid_argument("term_append: more than 2^30 bytes");
        if ((mtu & 31) || mtu < 64 || mtu > 65504) throw std::invalid_argument("term_append: mtu is a multiple of 32 in [64, 65504]");
        if (effective_max_message_length(len) > (1ull << 30)) throw std::invalid_argument("term_append: max_message_length above 2^30");
    }
};
struct TermAppendResult {
    std::size_t appended = 0;              // records that went in; the caller goes on with the rest
    std::uint64_t next = 0;                // the tail (len after TRIPPED)
    std::uint32_t stop = 0;                // SBE_TERM_APPEND_*
    std::vector<std::uint64_t> rec_tail;   // [appended] the block offset behind each record
};
// required(L): bytes of block the frames of an L-byte record take
std::uint64_t term_frames_length(std::uint64_t len, std::uint32_t mtu);
// Records data[rec_off[i], rec_off[i+1]) of a data_len-byte buffer; never reads outside it.
TermAppendResult term_append(std::uint8_t* block, std::size_t len, std::size_t start, const std::uint8_t* data,
                             std::size_t data_len, const std::uint64_t* rec_off, std::size_t n,
                             const TermAppendOptions& options = {});
class TermAppender {
public:
    // Records data[rec_off[i], rec_off[i+1]), i < n, of a data_len-byte host buffer into block[start, len).
    TermAppendResult append(const std::uint8_t* data, std::size_t data_len, const std::uint64_t* rec_off, std::size_t n,
                            std::uint8_t* block, std::size_t len, std::size_t start, const TermAppendOptions& options = {});
    // Records first_record.. of the batch into block[start, len).
    TermAppendResult append_batch(const EncodedBatch& batch, std::size_t first_record, std::uint8_t* block, std::size_t len,
                                  std::size_t start, const TermAppendOptions& options = {});
};

// The subscriber's egress step (polling_worker -> poll -> handle_incoming_message -> commit_message ->
// send_commit_offset -> offer) as one enqueue: the raw egress block goes up once, sbe_term_poll and
// the four *_counted calls (decode, classify, emit, term append) run back to back on the stream
// with the message count and the frame count staying in device memory.  The host waits once for
// the kernels (the counts come back with that wait); the downloads whose sizes the counts give
// take two more waits, as poll_term_block's do: the offsets, statuses, frame records and tails,
// then the carry, the messages and the bytes written to the ingress block.  The result is defined by the classes above: the ingress block holds what
// TermAppender::append writes for the frames AutoCommitter::commit_and_send_batch (json_fallback,
// session frames, no mask) offers for MessageParser's parse of FragmentReassembler::poll_term_block's
// messages, but for the records the device leaves to the host (SBE_CE_HOST: escaped or non-string
// topics), which are reported in `host` and not sent; `next` and the kept carry are
// poll_term_block's.  The CommitManager is not touched: the caller commits from the messages.
struct EgressStepOptions {
    std::size_t limit = ~(std::size_t)0;  // fragments per poll
    std::int64_t leadership_term_id = 0;
    std::int64_t cluster_session_id = 0;
    std::function<std::uint64_t()> clock;  // read twice, as CommitSendOptions::clock
    TermAppendOptions append;
};
struct EgressStepResult {
    std::uint64_t poll_counts[6] = {0, 0, 0, 0, 0, 0};  // sbe_term_poll's: fragments, next, payload bytes, stop, messages, carry
    std::size_t next = 0;                  // where the poll stopped: the start of the next call
    std::size_t messages = 0;
    std::uint64_t frames = 0, frame_bytes = 0;  // the emit call's totals
    TermAppendResult appended;             // of the commit frames; appended < frames: go on in the next term
    std::vector<std::size_t> frame_record; // [frames] the message each frame commits, ascending
    std::vector<std::size_t> host;         // messages left to the host (SBE_CE_HOST), ascending
    std::vector<std::size_t> too_long;     // SBE_CE_E109_MESSAGE_ID
    std::vector<std::size_t> fallback_e100;  // SBE_CE_E100_FALLBACK
};
class EgressCommitter {
public:
    explicit EgressCommitter(std::string client_id, std::string fallback_topic = "default");
    // as AutoCommitter::set_message_identifier (std::length_error beyond 63 topics or 4096 bytes)
    void set_message_identifier(const std::string& topic, const std::string& identifier);
    // One step over block[start, len) into ingress[ingress_start, ingress_len).  `messages`, when
    // given, receives the polled messages (what poll_term_block returns), for the records in `host`.
    // Throws what the composed calls throw: std::invalid_argument for a block, start, ingress
    // length or ingress start that is no multiple of 32, a start behind its block, more than 2^30
    // bytes, a bad mtu or max_message_length (TermAppendOptions::check); std::length_error when the
    // identifiers or client_id exceed 4096 bytes.
    EgressStepResult poll_commit_append(const std::uint8_t* block, std::size_t len, std::size_t start, std::uint8_t* ingress,
                                        std::size_t ingress_len, std::size_t ingress_start,
                                        const EgressStepOptions& options = {}, EncodedBatch* messages = nullptr);
    std::size_t pending_bytes() const { return acc_.size(); }

private:
    std::string client_id_, fallback_;
    std::map<std::string, std::string> identifiers_;
    std::vector<std::uint8_t> acc_;
};

// include/aeron_cluster/order_types.hpp:16-66: the members Order::to_json, Order::validate and
// publish_order read (the reference class carries more; they play no part in either).
struct Order {
    std::string id;
    std::string client_order_uuid;
    std::string base_token;
    std::string quote_token;
    std::string side;
    double quantity = 0.0;
    std::int64_t customer_id = 0;
    std::string status = "CREATED";
    std::int64_t timestamp = 0;
    std::string identifier;
    // read by validate() only (defaults: order_types.hpp:28-49)
    std::string order_type = "LIMIT";
    std::string time_in_force = "GTC";
    double limit_price = 0.0;
    std::optional<double> stop_price;
    std::optional<std::int64_t> expiry_timestamp;
    // src/order_types.cpp:122-181 (one-record batch on the GPU)
    std::string to_json() const;
    // src/order_types.cpp:66-120: every failed check's message, in the reference's order (host code,
    // as in the reference; the batch publisher runs the same checks on the device)
    std::vector<std::string> validate() const;
};

// A batch of Orders → Order::to_json texts (payload) and the headers JSON publish_order builds
// beside them (src/cluster_client.cpp:308-323, messageId = message_ids[i]); record i of each is
// bytes[offsets[i], offsets[i+1]), ready to be TopicMessage payload / headers.
struct OrderJsonBatch {
    EncodedBatch payload;
    EncodedBatch headers;
};
OrderJsonBatch orders_to_json(const std::vector<Order>& orders, const std::vector<std::string>& message_ids);

// include/aeron_cluster/cluster_client.hpp:30-52
class ClusterClientException : public std::runtime_error {
public:
    explicit ClusterClientException(const std::string& message) : std::runtime_error(message) {}
};
class InvalidMessageException : public ClusterClientException {
public:
    explicit InvalidMessageException(const std::string& message)
        : ClusterClientException("Invalid message: " + message) {}
};

// ClusterClient::publish_order / publish_order_to_topic (src/cluster_client.cpp:300-372) minus the
// connection checks: validate, message id, messageType, both JSON texts, create_topic_message and
// the session frame (src/session_manager.cpp:1050-1144), the record handed to an
// offer_ingress-shaped sink.  Every form is one fused device call (sbe_publish_orders_batch).
struct OrderPublisherOptions {
    bool session_framed = true;        // the 32-B SessionMessageHeader first, as the live path sends
    bool reference_truncate8 = true;   // SBE_ENC_REF_TRUNCATE8: the 26+Σlen bytes create_topic_message returns
    std::int64_t leadership_term_id = 0;
    std::int64_t cluster_session_id = 0;
    // OrderUtils::generate_message_id("msg") (src/order_types.cpp:428-437): msg_<ns>_<10000..99999>
    std::function<std::string()> message_id;
    // the TopicMessage timestamp (high_resolution_clock nanoseconds, src/session_manager.cpp:1050-1115)
    std::function<std::uint64_t()> clock;
};
struct PublishedOrders {
    std::vector<std::string> message_ids;  // one per order, made whether or not the order is valid
    std::vector<std::uint8_t> status;      // SBE_ENC_OK, SBE_ENC_E109_*, SBE_PUB_INVALID_* (first message)
    std::vector<std::uint16_t> error_mask; // bit k: validate()'s message k
    std::size_t offered = 0;               // records the sink accepted (stops at the first refusal)
};
class OrderPublisher {
public:
    OrderPublisher(OfferFn offer, std::string default_topic, OrderPublisherOptions options = {});
    // Return the message id.  Throw InvalidMessageException("Order validation failed: " + errors[0])
    // (the _to_topic form: "Topic is empty" first) and ClusterClientException("Failed to publish
    // order message") when the sink refuses the record.  validate() runs on the host first, as in
    // the reference: an invalid order makes no message id, reads no clock and makes no device call.
    std::string publish_order(const Order& order);
    std::string publish_order_to_topic(const Order& order, const std::string& topic);
    // One device call for all orders; the valid records are offered in order.  Does not throw on an
    // invalid order or a refused offer: see status / offered.
    PublishedOrders publish_orders_batch(const std::vector<Order>& orders);
    PublishedOrders publish_orders_batch_to_topic(const std::vector<Order>& orders, const std::string& topic);
    // The message text of validate()'s message k for this order (k < SBE_PUB_INVALID_COUNT).
    static std::string validation_message(unsigned k, const Order& order);

private:
    OfferFn offer_;
    std::string default_topic_;
    OrderPublisherOptions opt_;
};

// Feeds every encoded record of a batch to an offer_ingress-shaped sink in order; returns the
// number accepted before the first refusal.
std::size_t offer_batch(const EncodedBatch& batch, const OfferFn& offer);

// true when a gfx950 device is usable (all entry points above need one).
bool gpu_codec_available();
// threads (the caller's included) that stage batches and build ParseResults: AERON_AMD_HOST_THREADS,
// default min(16, cores)
unsigned host_threads();

// Stops the calling thread's small-batch serve kernel if it is resident (it exits after
// AERON_AMD_SERVE_IDLE_US without a call, default 1 ms; the next small call relaunches it).  While
// resident it holds a hardware queue that other streams of the process may share, and a
// device-wide synchronisation (hipDeviceSynchronize, torch.cuda.synchronize()) waits for it to go
// idle: call this before such a synchronisation, or before handing the GPU to other work.
void quiesce();

// Page-locks a long-lived host buffer (e.g. an Aeron term buffer mapped from /dev/shm) for the
// device's copy engines: batches decoded from registered (or hipHostMalloc'd) memory are copied to
// HBM in place, without the staging copy.  The memory stays registered until host_unregister.
void host_register(const void* p, std::size_t len);
void host_unregister(const void* p);

}  // namespace aeron_cluster
