/*
 * sbecodec.h — C ABI of the MI355X-native batch SBE record codec.
 *
 * This is the drop-in boundary for the wire codec of reverb-sys/aeron-cluster-client-cpp
 * (reference snapshot mounted at /root/reference; all file:line citations are relative to it).
 * Every entry point is plain C: pointers, sizes and integers only.  Device pointers are HIP
 * device (or host-pinned, device-visible) pointers; `stream` is a hipStream_t passed as void*
 * (NULL = the default stream).  Nothing here allocates, synchronises or copies on the host:
 * every call is an asynchronous launch on `stream` and returns after argument validation.
 * Every launch and memset of a call goes to `stream` and to no other stream.  A call writes the
 * output elements its comment names and nothing else: no byte before or after an output array,
 * and no byte outside the workspace size it asks for.  A workspace needs no particular contents:
 * a call writes every workspace word before it reads it (a workspace serves one stream at a time).
 * Offset arrays (rec_off, frag_off) need not start at 0: they index `in`, so records a..b of a
 * larger batch are processed by passing rec_off + a with n = b - a (and in_bytes = rec_off[b] -
 * rec_off[a]); the per-record outputs of that call start at element 0 of the arrays it is given
 * (status + a, view_off + 5 a, ... to fill the larger batch's arrays in place).
 *
 * Entry point                     replaces (reference)
 * ------------------------------  ------------------------------------------------------------
 * sbe_encode_topic_batch()        SBEEncoder::encode_topic_message   src/sbe_encoder.cpp:131-167
 *                                  (decl include/aeron_cluster/sbe_messages.hpp:158-164), its live
 *                                  twin SessionManager::Impl::create_topic_message
 *                                  src/session_manager.cpp:1050-1115 and the correct-length encoder
 *                                  inside ClusterClient::publish_topic src/cluster_client.cpp:1809-1864;
 *                                  output records are what ClusterClient::offer_ingress
 *                                  (include/aeron_cluster/cluster_client.hpp:409,
 *                                  src/cluster_client_offer.cpp:11-20) receives one by one.
 * sbe_encode_session_batch()      SessionManager::Impl::publish_message's frame: create_topic_message
 *                                  src/session_manager.cpp:1050-1115 behind the 32-B
 *                                  SessionMessageHeader that send_combined_message prepends
 *                                  (:936-967 build, :1018-1046 update, :1118-1144 combine).
 * sbe_encode_lite_batch()         CommitManager::build_commit_offset_message's CommitOffsetLite
 *                                  encoder src/commit_manager.cpp:107-132 (template 301) and the
 *                                  OrderRequestLite / OrderNotificationLite flyweights (201 / 202,
 *                                  include/model/OrderRequestLite.h:114-118, :1020-1050).
 * sbe_decode_batch(LITE)          the Lite templates' generated decode flyweights
 *                                  (wrapForDecode + fixed fields + getXAsString in order,
 *                                  include/model/CommitOffsetLite.h, OrderRequestLite.h,
 *                                  OrderNotificationLite.h).
 * sbe_reassemble_fragments()      LocalFragmentReassembler::onFragment src/cluster_client.cpp:39-82
 *                                  (BEGIN / END flag reassembly of Aeron fragments, before parse).
 * sbe_decode_batch(PARSE_MESSAGE) MessageParser::parse_message      src/sbe_encoder.cpp:513-551
 *                                  (+ parse_topic_message :724-831, decode_acknowledgment_with_sbe
 *                                  :833-954, decode_topic_message_with_sbe :957-1143,
 *                                  parse_session_event :618-647) → ParseResult
 *                                  include/aeron_cluster/sbe_messages.hpp:306-412
 * sbe_classify_commits()          the commit decision of ClusterClient::handle_incoming_message
 *                                  src/cluster_client.cpp:1198-1303: should_skip_auto_commit :847-886,
 *                                  extract_topic_from_message :756-806, and the last commit per
 *                                  topic that CommitManager::commit_message keeps
 *                                  (src/commit_manager.cpp:29-35)
 * sbe_emit_commit_offsets()       the other half of commit_message src/cluster_client.cpp:626-633:
 *                                  send_commit_offset :1264-1278, i.e. build_commit_offset_message
 *                                  src/commit_manager.cpp:107-132 behind send_combined_message's session
 *                                  header :678-682, for the records sbe_classify_commits committed
 * sbe_decode_batch(ON_EGRESS)     decode_ack  src/ack_decoder.cpp:29-105 (AckInfo
 *                                  include/aeron_cluster/ack_decoder.hpp:9-15) and
 *                                  MessageHandler::on_egress include/aeron_cluster/message_handler.hpp:35-68
 * sbe_order_to_json_batch()       Order::to_json src/order_types.cpp:122-181 and publish_order's
 *                                  headers JSON src/cluster_client.cpp:308-323 (the strings that
 *                                  become the TopicMessage payload / headers)
 * sbe_publish_orders_batch()      ClusterClient::publish_order / publish_order_to_topic
 *                                  src/cluster_client.cpp:300-372 in one call: Order::validate
 *                                  src/order_types.cpp:66-120, the messageType choice, both JSON texts,
 *                                  create_topic_message and the session frame
 *                                  src/session_manager.cpp:1050-1144 (sbe_publish_orders_workspace_size,
 *                                  sbe_publish_orders_output_bound size its buffers)
 * sbe_inflight_remember()         ClusterClient::remember_outgoing src/cluster_client.cpp:1920-1922 for
 *                                  the records publish_topic offered (:1860-1861): the emplace into
 *                                  inflight_ (include/aeron_cluster/cluster_client.hpp:420)
 * sbe_inflight_match_acks()       ClusterClient::on_ack_default src/cluster_client.cpp:1924-1941, the
 *                                  ack callback wired at :1648: find / erase in inflight_ and the time
 *                                  the round trip is measured from (sbe_inflight_init, _rehash,
 *                                  _table_size, _workspace_size manage the device table)
 * sbe_inflight_note_keys()        the received_message_ids / received_client_order_ids bookkeeping of the
 *                                  subscriber's callback, examples/pubsub_reconnect_test.cpp:625-667
 *                                  (again from :1190): insert-if-new, already_processed and the
 *                                  per-id count of record_duplicate_delivery (:83-90)
 * sbe_inflight_lookup_keys()      the correlation with the publisher, :669-691: was_sent and the
 *                                  latency recorded once per client_order_id, against the ids
 *                                  sbe_inflight_remember stored (:455-459, :498-501)
 *                                  (sbe_inflight_reset_values: clear_duplicate_tracking, :70-73)
 * sbe_delivery_keys()             the three keys of those lookups per record: message_id and the
 *                                  client_order_id / order_id the callback picks, :592-619
 * sbe_order_select()              the test in front of them, :578-579: ParseResult::is_order_message /
 *                                  is_topic_message / is_session_event / is_acknowledgment
 *                                  include/aeron_cluster/sbe_messages.hpp:332-406 per record, and
 *                                  classify_topic include/aeron_cluster/topic_router.hpp
 * sbe_term_scan()                 no reference source (third-party Aeron, TermReader::read): the walk
 *                                  over the 32-byte data-frame headers of a term-buffer block that
 *                                  hands fragments to onFragment src/cluster_client.cpp:39-82
 * sbe_term_poll()                 that walk and onFragment src/cluster_client.cpp:39-82 in one call: a
 *                                  raw block and the open accumulator in, whole messages out, the
 *                                  fragment count handed on in device memory and every payload byte
 *                                  copied once (sbe_term_poll_workspace_size)
 * sbe_term_append()               no reference source (third-party Aeron, ExclusivePublication::offer ->
 *                                  ExclusiveTermAppender): the data frames, fragmented at the MTU, and
 *                                  the end-of-term padding frame that the per-record offer behind
 *                                  offer_ingress src/cluster_client_offer.cpp:11-20 writes into a term,
 *                                  for a whole encoded batch (sbe_term_frames_length,
 *                                  sbe_term_append_workspace_size, sbe_term_append_tile)
 * sbe_inflight_list_keys()        printMessageComparison examples/pubsub_reconnect_test.cpp:130-204 and
 *                                  printClientOrderAudit :206-274: the ids sent and never received, or
 *                                  received and never sent, the first ones in std::set order; with a
 *                                  least value of 2, the ids of duplicate_delivery_counts (:83-90)
 * sbe_latency_append()            the latency the callback records per client_order_id (:669-691), kept
 *                                  in a device log (sbe_latency_log_size, _log_init)
 * sbe_latency_report()            printLatencyReport :276-353: the sorted latencies, sum, min, max and
 *                                  the percentiles by its own rank formula (:322-326)
 * sbe_json_extract_batch()        what a consumer's callback reads out of result.payload: the
 *                                  Json::parseFromStream + isMember / operator[] lookups of
 *                                  examples/pubsub_reconnect_test.cpp:576-620 (again :1142-1160) and of
 *                                  CommitManager::parse_commit_offset src/commit_manager.cpp:177-195,
 *                                  for a table of member paths over a whole batch
 * sbe_serve_*()                   the same encoders / decoders for small batches (one record per
 *                                  call, as the reference's per-message API is used: parse_message per
 *                                  fragment src/cluster_client.cpp:1185, publish_topic per message)
 *                                  through a resident serve kernel instead of a launch per call
 * sbe_gather_encoded()            no reference counterpart (its transport is Aeron,
 *                                  src/session_manager.cpp:1180): the RCCL gather of encoded shards
 *                                  to one ingress rank
 */
#ifndef SBECODEC_H
#define SBECODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBECODEC_ABI_VERSION 8

/* ---- return codes of every entry point ---- */
#define SBE_OK 0
#define SBE_EINVAL (-1)    /* bad argument (null pointer, n too large, bad mode) */
#define SBE_EHIP (-2)      /* a HIP launch failed (hipGetLastError != hipSuccess) */
#define SBE_ENOSPC (-3)    /* workspace too small */
#define SBE_ENODEV (-4)    /* no gfx950 device visible */

/* ---- wire constants (include/model/MessageHeader.h:95-490, TopicMessage.h:114-118,
 *      Acknowledgment.h:114-118, include/aeron_cluster/config.hpp:169-199) ---- */
#define SBE_HEADER_LEN 8u
#define SBE_TM_BLOCK_LEN 16u
#define SBE_TM_TEMPLATE_ID 1u
#define SBE_ACK_TEMPLATE_ID 2u
#define SBE_TOPIC_SCHEMA_ID 1u
#define SBE_CLUSTER_SCHEMA_ID 111u
#define SBE_SESSION_EVENT_TEMPLATE_ID 2u
#define SBE_TM_FIELDS 5u           /* topic, messageType, uuid, payload, headers */
#define SBE_TM_WIRE_OVERHEAD 34u   /* 8 header + 16 block + 5 x u16 length */
#define SBE_TM_REF_OVERHEAD 26u    /* reference encode_topic_message emits 8 B less */
#define SBE_VAR_MAX_LEN 65534u     /* TopicMessage.h:1396-1428 (E109 above this) */
#define SBE_SESSION_HDR_LEN 32u    /* SessionMessageHeader {24,1,111,8} + termId, sessionId, ts=0
                                      (src/session_manager.cpp:936-967) */
#define SBE_SESSION_BLOCK_LEN 24u
#define SBE_SESSION_TEMPLATE_ID 1u
#define SBE_CLUSTER_SCHEMA_VERSION 8u
#define SBE_LITE_BLOCK_LEN 12u     /* u32 topicId @0, u64 sequence @4 (CommitOffsetLite.h:114, :337-420) */
#define SBE_ORDER_REQUEST_LITE_TEMPLATE_ID 201u      /* uuid, messageIdentifier, payload */
#define SBE_ORDER_NOTIFICATION_LITE_TEMPLATE_ID 202u /* uuid, messageIdentifier, payload */
#define SBE_COMMIT_OFFSET_LITE_TEMPLATE_ID 301u      /* messageId, messageIdentifier */

/* ===================================== encode ===================================== */

/* encode flags */
#define SBE_ENC_REF_TRUNCATE8 0x1u /* emit exactly what SBEEncoder::encode_topic_message returns:
                                      buffer.resize(encodedLength()) keeps only the first
                                      26+Σlen bytes of the wire record (src/sbe_encoder.cpp:163-164) */
#define SBE_ENC_PUBLISH_TOPIC 0x2u /* the encoder block of ClusterClient::publish_topic
                                      (src/cluster_client.cpp:1823-1858): wire length, and the
                                      put*(const char*, int) overloads (TopicMessage.h:515-529) that
                                      take the length as std::uint16_t: a field of L bytes writes
                                      length L mod 65536 followed by its first L mod 65536 bytes; no
                                      E109 (computeLength is never called).  Topic batches only; not
                                      with SBE_ENC_REF_TRUNCATE8.  The caller supplies the uuid
                                      ("pub_" + now_nanos(), :1818) and "{}" for empty headers (:1821),
                                      as the host mirror's publish_topic does. */

/* Lite records: 8 header {12, template, 1, 1} + 12 block + nf x (u16 length + bytes), nf = 2
 * (301) or 3 (201, 202).  Wire overhead 20 + 2 nf; no truncation (8 + encodedLength() is the
 * whole record, src/commit_manager.cpp:129-130). */
#define SBE_LITE_OVERHEAD(nf) (20u + 2u * (nf))

/* per-record encode status */
#define SBE_ENC_OK 0u
#define SBE_ENC_E109_TOPIC 1u        /* "topicLength too long for length type [E109]" */
#define SBE_ENC_E109_MESSAGE_TYPE 2u /* "messageTypeLength too long for length type [E109]" */
#define SBE_ENC_E109_UUID 3u         /* "uuidLength too long for length type [E109]" */
#define SBE_ENC_E109_PAYLOAD 4u      /* "payloadLength too long for length type [E109]" */
#define SBE_ENC_E109_HEADERS 5u      /* "headersLength too long for length type [E109]" */
#define SBE_ENC_OVERFLOW 6u          /* record does not fit in out_capacity (nothing written: no byte of
                                        out from the end of the last record that fits is touched) */
/* Lite templates: status 1 + f = "<field f>Length too long for length type [E109]" with the
 * template's field names in wire order (computeLength, e.g. CommitOffsetLite.h:839-870). */

/* A batch of TopicMessages in struct-of-arrays form.  Field order per record is the wire order
 * topic, messageType, uuid, payload, headers (TopicMessage.h:515-1231).
 *   arena      string bytes.
 *   str_off    [n][5] byte offsets into arena, or NULL: "packed" — the strings of record 0..n-1
 *              lie back to back in arena in record-major, field-minor order from arena[0].
 *   str_len    [n][5] lengths (> 65534 → E109, the record emits no bytes).
 *   timestamp  [n]; 0 is replaced by ts_default (the reference substitutes the wall clock for 0,
 *              src/sbe_encoder.cpp:134-138; the caller passes that clock value). */
typedef struct sbe_tm_batch {
    const uint8_t* arena;
    const uint32_t* str_off;
    const uint32_t* str_len;
    const uint64_t* timestamp;
} sbe_tm_batch;

/* Bytes of device workspace sbe_encode_topic_batch needs for n records (look-back tile state). */
size_t sbe_encode_workspace_size(uint64_t n);

/* Optional: zero a workspace (hipMemsetAsync on `stream`).  The encoder needs no particular
 * workspace contents; a workspace serves one stream at a time. */
int sbe_encode_workspace_init(void* workspace, size_t workspace_bytes, void* stream);

/* Upper bound of the encoded stream for a batch whose strings total `string_bytes`. */
uint64_t sbe_encode_output_bound(uint64_t n, uint64_t string_bytes, uint32_t flags);

/* Encode n TopicMessages into one packed byte stream.
 *   out        device buffer of out_capacity bytes; record i is out[out_off[i] .. out_off[i+1]).
 *   out_off    [n+1] u64 device array (written).
 *   status     [n] u8 device array (written) or NULL.
 *   workspace  device memory of >= sbe_encode_workspace_size(n) bytes, 16-B aligned.
 *   alignment  out 16 B, out_off 8 B (arena, str_off, str_len, timestamp: natural alignment).
 * Records are independent; a failing record (E109, overflow) emits 0 bytes and the batch goes on. */
int sbe_encode_topic_batch(const sbe_tm_batch* in, uint64_t n, uint64_t ts_default, uint32_t flags,
                           uint8_t* out, uint64_t out_capacity, uint64_t* out_off, uint8_t* status,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Session-framed encode: every record is the 32-B SessionMessageHeader
 *   {blockLength 24, templateId 1, schemaId 111, version 8, i64 leadershipTermId,
 *    i64 clusterSessionId, i64 timestamp 0}
 * followed by the TopicMessage exactly as sbe_encode_topic_batch emits it under `flags`
 * (SBE_ENC_REF_TRUNCATE8: the 26+Σlen bytes create_topic_message returns, which is what the live
 * publish path sends; 0: the wire-correct 34+Σlen).  Record i = out[out_off[i]..out_off[i+1]) is
 * one Publication::offer of send_combined_message.  Workspace, alignment and status as for
 * sbe_encode_topic_batch. */
int sbe_encode_session_batch(const sbe_tm_batch* in, uint64_t n, uint64_t ts_default, uint32_t flags,
                             int64_t leadership_term_id, int64_t cluster_session_id, uint8_t* out,
                             uint64_t out_capacity, uint64_t* out_off, uint8_t* status, void* workspace,
                             size_t workspace_bytes, void* stream);

/* A batch of Lite records (struct of arrays):
 *   arena, str_off ([n][nf] or NULL = packed), str_len [n][nf]: the var strings in wire order;
 *   topic_id [n]: u32 topicId; sequence [n]: u64 sequence. */
typedef struct sbe_lite_batch {
    const uint8_t* arena;
    const uint32_t* str_off;
    const uint32_t* str_len;
    const uint32_t* topic_id;
    const uint64_t* sequence;
} sbe_lite_batch;

/* Fields per record of a Lite template (2 or 3), 0 if template_id is not one of them. */
uint32_t sbe_lite_fields(uint32_t template_id);

/* Upper bound of the encoded stream of a Lite batch whose strings total `string_bytes`. */
uint64_t sbe_lite_output_bound(uint64_t n, uint64_t string_bytes, uint32_t template_id);

/* Encode n Lite records of template_id (201, 202 or 301).  Outputs, workspace and alignment as
 * for sbe_encode_topic_batch (the same workspace size). */
int sbe_encode_lite_batch(const sbe_lite_batch* in, uint64_t n, uint32_t template_id, uint8_t* out,
                          uint64_t out_capacity, uint64_t* out_off, uint8_t* status, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ===================================== decode ===================================== */

#define SBE_DEC_PARSE_MESSAGE 0u /* MessageParser::parse_message semantics → ParseResult */
#define SBE_DEC_ON_EGRESS 1u     /* MessageHandler::on_egress semantics (decode_ack first) */
#define SBE_DEC_LITE 2u          /* Lite-template flyweight decode (201 / 202 / 301) */

/* per-record decode status.  Parse mode (0..31): */
#define SBE_ST_TM 0u                 /* TopicMessage: views topic,type,uuid,payload,headers */
#define SBE_ST_ACK 1u                /* Acknowledgment (printable-run heuristic): views 0..2 */
#define SBE_ST_SESSION_EVENT 2u      /* SessionEvent: view 3 = detail (u32-prefixed) */
#define SBE_ST_ERR_NULL_EMPTY 16u    /* "Null or empty data" */
#define SBE_ST_ERR_HEADER 17u        /* "Failed to decode message header" */
#define SBE_ST_ERR_UNKNOWN_TYPE 18u  /* "Unknown message type: template=T, schema=S" (hdr kept) */
#define SBE_ST_ERR_SESSION_EVENT 19u /* "Failed to decode SessionEvent" */
#define SBE_ST_ERR_SESSION_SHORT 20u /* "Session message too short to contain embedded message" */
#define SBE_ST_ERR_EMBEDDED_SHORT 21u /* "Embedded message too short" */
#define SBE_ST_ERR_EMBEDDED_TEMPLATE 22u /* "Unknown embedded message template_id: <param>" */
#define SBE_ST_ERR_EMBEDDED_SCHEMA 23u   /* "Unknown embedded message schema_id: <param>" */
#define SBE_ST_ERR_DIRECT_TEMPLATE 24u   /* "Unknown direct message template_id: <param>" */
#define SBE_ST_ERR_TM_E100 25u       /* "SBE TopicMessage decoding failed: buffer too short [E100]" */
#define SBE_ST_ERR_ACK_SHORT 26u     /* "Buffer too short for Acknowledgment message. Need at least
                                         16 bytes, got <param>" */
/* On-egress mode (32..): */
#define SBE_ST_EG_ACK_SIMPLE 32u     /* decode_ack simple 16-B control ack; ts = timestamp_nanos */
#define SBE_ST_EG_ACK 33u            /* decode_ack full ack; views messageId,topic,correlationId */
#define SBE_ST_EG_TM 34u             /* topic-message callback; views topic,type,uuid,payload,headers */
#define SBE_ST_EG_NONE 35u           /* on_egress returns without a callback */
#define SBE_ST_EG_THROW_E100 36u     /* on_egress throws std::runtime_error("buffer too short [E100]") */
/* Lite mode (48..): the generated flyweight sequence MessageHeader::wrap, wrapForDecode(buf, 8,
 * blockLength, version, len), topicId(), sequence(), getXAsString() per var field in order. */
#define SBE_ST_LITE 48u              /* decoded: ts = sequence, view_off[4] = topicId, views 0..nf-1 */
#define SBE_ST_LITE_E100 49u         /* a flyweight bounds check threw "buffer too short [E100]" (also:
                                         the 12 fixed bytes lie past the record) */
#define SBE_ST_LITE_NOT_LITE 50u     /* len < 8, schema != 1 or template not 201/202/301 (hdr kept
                                         when len >= 8) */

/* per-record decode flags */
#define SBE_FL_ID_DEFAULT 0x1u      /* ack: message_id = "ack_" + decimal(ts) */
#define SBE_FL_PAYLOAD_DEFAULT 0x2u /* ack: payload = "SUCCESS" */
#define SBE_FL_HEADERS_E100 0x4u    /* TM: headers read hit E100 and was swallowed (headers = "") */
#define SBE_FL_SEQ_KEY 0x8u         /* TM: payload (>= 16 B) contains the bytes "_sequence_number" */
#define SBE_FL_WRAPPED 0x10u        /* record was a schema-111 session message (embedded decode) */
#define SBE_FL_SEQ_ESC 0x20u        /* TM: payload (>= 16 B) contains a '\\' byte (a key spelled with
                                       \u escapes decodes to "_sequence_number" without containing it) */
/* A TM record without SEQ_KEY and SEQ_ESC has ParseResult.sequence_number == 0 under any JSON
 * parser; sbe_eval_sequence_numbers evaluates the others. */

/* Decoded records, struct of arrays, all device arrays of n (or n*4 / n*5) elements.
 *   hdr      [n][4] block_length, template_id, schema_id, version as ParseResult reports them.
 *   ts       [n] ParseResult.timestamp / AckInfo.timestamp_nanos.
 *   view_off [n][5], view_len [n][5]: byte ranges relative to the record's first byte.
 *            For statuses with a parameter, view_off[i*5] holds it. */
typedef struct sbe_decoded {
    uint8_t* status;
    uint8_t* flags;
    uint16_t* hdr;
    uint64_t* ts;
    uint32_t* view_off;
    uint32_t* view_len;
    uint64_t* seq; /* optional (NULL: skip), parse mode only: seq[i] = ParseResult.sequence_number of
                      every TopicMessage flagged SBE_FL_SEQ_KEY / SBE_FL_SEQ_ESC, evaluated in the same
                      launch (see sbe_eval_sequence_numbers); other entries are not written (8-B aligned) */
} sbe_decoded;

/* Decode n records; record i is in[rec_off[i] .. rec_off[i+1]) (rec_off: [n+1] device u64).
 * Record boundaries come from the transport (Aeron fragments, src/cluster_client.cpp:541-546):
 * the SBE header carries no total length.  Alignment: in 16 B, rec_off/hdr/ts 8 B, views 4 B. */
int sbe_decode_batch(const uint8_t* in, const uint64_t* rec_off, uint64_t n, uint32_t mode,
                     const sbe_decoded* out, void* stream);

/* sbe_decode_batch with the batch's total record bytes (rec_off[n] - rec_off[0]) as the caller
 * knows them, used only to pick the kernel shape (the LDS window of a 64-record tile, which caps
 * the workgroups per CU): records over 320 B on average (long payloads) 13 KiB windows, over 256 B
 * (session frames) 12 KiB (a tile takes two or more); up to 112 B 8 KiB; up to 204 B 15 KiB;
 * others 16 KiB.
 * in_bytes = 0: the 16 KiB kernel.  Outputs are identical either way. */
int sbe_decode_batch_sized(const uint8_t* in, const uint64_t* rec_off, uint64_t n, uint64_t in_bytes, uint32_t mode,
                           const sbe_decoded* out, void* stream);

/* ParseResult.sequence_number (src/sbe_encoder.cpp:1031-1125) as a separate launch, for
 * descriptors decoded with seq == NULL: for every record that
 * sbe_decode_batch(SBE_DEC_PARSE_MESSAGE) left with status SBE_ST_TM and flag SBE_FL_SEQ_KEY or
 * SBE_FL_SEQ_ESC, parse its payload with the semantics of jsoncpp 1.9.5's CharReaderBuilder
 * defaults (comments and trailing commas allowed, extra content after the root ignored, stack
 * limit 1000, UTF-8 BOM skipped) and write seq[i] = the first non-zero "_sequence_number" of
 * root, root.message, root.message.message, root.message.message.message (extractSequence:
 * integers as u64, other numbers through a correctly rounded double and the x86-64 cast, strings
 * through std::stoull), or 0 when the payload does not parse.  seq[i] of any other record is not
 * written: its sequence_number is 0.  in / rec_off / status / flags / view_* are the arguments and
 * outputs of that decode call; seq is a device u64[n] (8-B aligned).  Same stream order rules. */
int sbe_eval_sequence_numbers(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const sbe_decoded* dec,
                              uint64_t* seq, void* stream);

/* MATERIALIZE: the five views of every decoded record copied out of the input into one arena, so
 * that the strings outlive the input buffer, as the reference's ParseResult owns its std::strings
 * (include/aeron_cluster/sbe_messages.hpp:306-328) and a poll callback's fragment dies with the
 * callback (src/cluster_client.cpp:541-546).  After sbe_decode_batch[_sized] on the same in /
 * rec_off (dec: its outputs), view k of record i goes to arena[arena_off[5 i + k] ..) with
 * view_len[i][k] bytes, views in record order and back to back (arena_off: device u64 [5 n + 1],
 * the last entry the total; a view of length 0, including the Lite topicId slot, takes no bytes).
 * A view that would end past arena_capacity is not written (arena_off still holds the full
 * layout, so the caller can size the arena from arena_off[5 n] and rerun); nothing is written past
 * arena_capacity: the views written are a prefix of the layout, and the arena is untouched from
 * the end of the last view written.  dec->status must be non-null and is not read: every record is
 * copied by the view_len its decode left, whatever its status (a record the decode rejected has
 * the lengths that decode wrote for it).  Alignment: rec_off / arena_off 8 B, view_off / view_len
 * 4 B (SBE_EINVAL otherwise, before any launch); in and arena need none.  Workspace:
 * sbe_materialize_workspace_size(n) bytes (16-B aligned). */
size_t sbe_materialize_workspace_size(uint64_t n);
int sbe_materialize_views(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const sbe_decoded* dec,
                          uint8_t* arena, uint64_t arena_capacity, uint64_t* arena_off, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ============================ auto-commit classification ============================ */
/* The second half of ClusterClient::handle_incoming_message (src/cluster_client.cpp:1198-1303)
 * for a decoded batch: should_skip_auto_commit (:847-886), extract_topic_from_message (:756-806)
 * and the commit test (:1251), per record, after sbe_decode_batch(SBE_DEC_PARSE_MESSAGE) on the
 * same in / rec_off (dec: its outputs).  cm[i] is the first clause that fires, in the reference's
 * order: */
#define SBE_CM_COMMIT 0u             /* reaches commit_message (given a successful callback: the host's business) */
#define SBE_CM_NOT_PARSED 1u         /* status >= 16 (result.success false) */
#define SBE_CM_SKIP_TYPE 2u          /* message_type is one of the six literals (:849-854); every SBE_ST_ACK */
#define SBE_CM_SKIP_ACK_ID 3u        /* message_id starts with "ack_" (:859) */
#define SBE_CM_SKIP_TOPIC 4u         /* the extracted topic is "_ack" or "_subscriptions" */
#define SBE_CM_SKIP_CONTROL 5u       /* topic "_control", message_type not REPLAY_COMPLETE and no
                                        "REPLAY_COMPLETE" in the payload bytes (:871-878) */
#define SBE_CM_SKIP_EMPTY_PAYLOAD 6u /* empty payload (:881; not reached by a _control REPLAY_COMPLETE) */
#define SBE_CM_NO_ID 7u              /* not skipped, but message_id is empty (:1251); every
                                        SBE_ST_SESSION_EVENT (message_id is never set there, so what
                                        should_skip_auto_commit returns cannot be observed) */
/* where the topic came from (extract_topic_from_message); NONE: extraction did not run (the
 * record stopped at an earlier clause, or is not a TopicMessage) */
#define SBE_TOPIC_SRC_NONE 0u
#define SBE_TOPIC_SRC_HEADERS 1u         /* headers.topic */
#define SBE_TOPIC_SRC_PAYLOAD 2u         /* payload.topic */
#define SBE_TOPIC_SRC_PAYLOAD_MESSAGE 3u /* payload.message.topic */
#define SBE_TOPIC_SRC_FALLBACK 4u        /* the caller's topic, table entry 0 (*subscribed_topics_.begin() or "default") */
/* what the topic token is; the host applies Value::asString to the non-string kinds */
#define SBE_TOPIC_KIND_NONE 0u       /* no token (sources NONE and FALLBACK) */
#define SBE_TOPIC_KIND_STRING 1u     /* no backslash: the range is the topic verbatim */
#define SBE_TOPIC_KIND_STRING_ESC 2u /* the host decodes the escapes */
#define SBE_TOPIC_KIND_NUMBER 3u     /* asString: decimal or "%.17g" text */
#define SBE_TOPIC_KIND_TRUE 4u       /* "true" */
#define SBE_TOPIC_KIND_FALSE 5u      /* "false" */
#define SBE_TOPIC_KIND_NULL 6u       /* "" */
#define SBE_TOPIC_UNKNOWN 0xFFFFFFFFu /* no table entry equals the topic; also every non-commit record */
#define SBE_TOPIC_HOST 0xFFFFFFFEu    /* a non-string kind: the host converts and looks it up */
#define SBE_COMMIT_MAX_TOPICS 64u
#define SBE_COMMIT_TABLE_BYTES 4096u

/* Outputs, device arrays.  topic_off / topic_len: the topic token relative to the record's first
 * byte (strings: between the quotes; numbers and literals: the token), 0 for sources NONE and
 * FALLBACK.  topic_idx: for SBE_CM_COMMIT records the first table entry equal to the decoded
 * topic (FALLBACK: 0), SBE_TOPIC_UNKNOWN or SBE_TOPIC_HOST; SBE_TOPIC_UNKNOWN for every other
 * record.  last [k]: the largest SBE_CM_COMMIT record index per table entry (UINT64_MAX: none).
 * count [k + 2]: SBE_CM_COMMIT records per entry, then those with SBE_TOPIC_UNKNOWN, then those
 * with SBE_TOPIC_HOST. */
typedef struct sbe_commit_out {
    uint8_t* cm;         /* [n] */
    uint8_t* topic_src;  /* [n] */
    uint8_t* topic_kind; /* [n] */
    uint32_t* topic_off; /* [n] */
    uint32_t* topic_len; /* [n] */
    uint32_t* topic_idx; /* [n] */
    uint64_t* last;      /* [k] */
    uint64_t* count;     /* [k + 2] */
} sbe_commit_out;

/* Workspace bytes sbe_classify_commits needs (0: none; workspace may then be NULL). */
size_t sbe_commit_workspace_size(uint64_t n, uint32_t k);

/* Classify n decoded records.  The topic table: k entries (1..SBE_COMMIT_MAX_TOPICS), entry j =
 * topic_arena[topic_off[j] .. topic_off[j+1]) (topic_off: device u32 [k + 1]); entry 0 is the
 * fallback topic.  topic_arena must be readable for SBE_COMMIT_TABLE_BYTES bytes: the host does not
 * read topic_off, the kernel clamps every offset to that size (and an entry whose end lies before
 * its start to length 0), so it stays inside the arena whatever topic_off holds.  The call sets
 * last and count itself on `stream` (two calls in a row give the same result); n == 0 is SBE_OK
 * with both initialised: only out, out->last, out->count and k are checked then, the per-record
 * arrays and the topic table are not looked at and may be null.  SBE_EINVAL (nothing written): a
 * null pointer, k == 0 or k > SBE_COMMIT_MAX_TOPICS, a u32 array not 4-byte or a u64 array not
 * 8-byte aligned. */
int sbe_classify_commits(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const sbe_decoded* dec,
                         const uint8_t* topic_arena, const uint32_t* topic_off, uint32_t k,
                         const sbe_commit_out* out, void* workspace, size_t workspace_bytes, void* stream);

/* ============================== JSON members by path ============================== */
/* The members a consumer reads out of a decoded JSON document (the payload or the headers of a
 * TopicMessage, or a bare document), for a caller-given table of member paths and every record of
 * a batch in one launch.  A path is 1..SBE_JSON_MAX_DEPTH member names, e.g. message / message /
 * order_details / client_order_id; a table holds 1..SBE_JSON_MAX_PATHS distinct paths.  Names are
 * the decoded member names: raw bytes, 1..SBE_JSON_MAX_NAME each, SBE_JSON_NAME_BYTES in all.
 *
 * The document is parsed as Json::parseFromStream / CharReader::parse with CharReaderBuilder
 * defaults parse it (jsoncpp 1.9.5; the reader sbe_eval_sequence_numbers and sbe_classify_commits
 * use): comments and trailing commas allowed, a BOM skipped, a NUL ends the stream, content after
 * the root ignored, stack limit 1000, a later duplicate key replaces the earlier value.  doc[i]: */
#define SBE_JX_OK 0u            /* the root parsed; root_kind[i] says what it is */
#define SBE_JX_NOT_SELECTED 1u  /* select[i] == 0, or (with descriptors) the record is not an SBE_ST_TM */
#define SBE_JX_EMPTY 2u         /* a zero-byte document (every reference caller tests .empty() first); also
                                   view 4 under SBE_FL_HEADERS_E100 */
#define SBE_JX_FAILED 3u        /* the parse returns false */
#define SBE_JX_STACK 4u         /* the reader throws "Exceeded stackLimit in readValue()" */
/* Everything but SBE_JX_OK leaves root_kind and every path SBE_JX_MISSING.
 * kind[i][p], per record and path (1..6 are the SBE_TOPIC_KIND_* values): */
#define SBE_JX_MISSING 0u
#define SBE_JX_STRING 1u        /* no backslash: the range is the string verbatim */
#define SBE_JX_STRING_ESC 2u    /* the host decodes the escapes */
#define SBE_JX_NUMBER 3u        /* a token the reader accepted as a number; the host converts it */
#define SBE_JX_TRUE 4u
#define SBE_JX_FALSE 5u
#define SBE_JX_NULL 6u
#define SBE_JX_OBJECT 7u
#define SBE_JX_ARRAY 8u
/* off / len are relative to the record's first byte.  Strings: the bytes between the quotes;
 * numbers and literals: the token; containers: from the opening bracket through the closing one
 * (jsoncpp's getOffsetStart() .. getOffsetLimit()); MISSING: 0, 0.  A path resolves through
 * objects only: when a prefix is missing or is not an object the path is MISSING (a caller who
 * must tell the two apart adds the prefix as a path of its own).  The last of several equal keys
 * wins at every level, also when it replaces an object by a scalar; member names are compared
 * after decodeString (a name spelled with escapes matches its decoded form).  No numeric values are
 * produced: number tokens are validated as the reader validates them and returned as ranges. */
#define SBE_JSON_MAX_PATHS 16u
#define SBE_JSON_MAX_DEPTH 4u
#define SBE_JSON_MAX_NAME 64u
#define SBE_JSON_NAME_BYTES 1024u

typedef struct sbe_json_paths { /* host memory, read during the call only */
    uint32_t n_paths;
    const uint8_t* depth;     /* [n_paths] names per path */
    const uint8_t* names;     /* the names of path 0, then of path 1, ..., back to back */
    const uint32_t* name_off; /* [sum of depth + 1] name j is names[name_off[j] .. name_off[j+1]) */
} sbe_json_paths;

typedef struct sbe_json_out { /* device arrays; P = n_paths */
    uint8_t* doc;       /* [n] SBE_JX_OK .. SBE_JX_STACK */
    uint8_t* root_kind; /* [n] */
    uint8_t* kind;      /* [n][P] */
    uint32_t* off;      /* [n][P] */
    uint32_t* len;      /* [n][P] */
} sbe_json_out;

/* Workspace bytes sbe_json_extract_batch needs (0: none; workspace may then be NULL). */
size_t sbe_json_extract_workspace_size(uint64_t n, uint32_t n_paths);

/* Extract the paths from n documents.  dec == NULL: record i, in[rec_off[i] .. rec_off[i+1]), is
 * the document itself, and view must be 0.  With dec (the outputs of
 * sbe_decode_batch(SBE_DEC_PARSE_MESSAGE) on the same in / rec_off) the document is view 3
 * (payload) or view 4 (headers) of every SBE_ST_TM record, kept inside its record whatever the
 * descriptors say.  select: NULL, or a device u8 [n] (0: the record is skipped).  The path table
 * travels in the launch arguments: the call reads no device table and makes no copy.  One launch
 * on `stream`; every element i < n of the five output arrays is written.  n == 0 is SBE_OK with
 * no launch.  SBE_EINVAL (before any launch, nothing written): a null pointer, a path table
 * outside the limits above, an empty name, the same path twice, a view that does not go with dec,
 * rec_off not 8-byte or a u32 array not 4-byte aligned. */
int sbe_json_extract_batch(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const sbe_decoded* dec,
                           uint32_t view, const uint8_t* select, const sbe_json_paths* paths,
                           sbe_json_out* out, void* workspace, size_t workspace_bytes, void* stream);

/* ============================== commit-offset frames ============================== */
/* The second half of ClusterClient::commit_message (src/cluster_client.cpp:626-633) for a batch
 * that sbe_decode_batch(SBE_DEC_PARSE_MESSAGE) and sbe_classify_commits have been over, with no
 * host round trip between them: for every committed record the frame send_commit_offset sends
 * (:1264-1278), compacted in record order.  A frame is
 *   [the 32-B SessionMessageHeader {24,1,111,8, termId, sessionId, 0} when `session`]
 *   header {12,301,1,1}, u32 topicId, u64 sequence, u16 + messageId, u16 + messageIdentifier
 * (CommitManager::build_commit_offset_message, src/commit_manager.cpp:107-132, behind
 * send_combined_message :678-682): topicId = topic_id[topic_idx[i]], messageId = view 2 of record
 * i (ParseResult.message_id), messageIdentifier = entry topic_idx[i] of the identifier table,
 * sequence = dec->seq[i] when dec->status[i] == SBE_ST_TM and dec->flags[i] has SBE_FL_SEQ_KEY or
 * SBE_FL_SEQ_ESC, else 0 (decode writes no other entry; dec->seq == NULL: 0 everywhere).
 * status[i], the first line that applies: */
#define SBE_CE_NONE 0u            /* plan->cm[i] != SBE_CM_COMMIT, or mask[i] == 0 (the callback failed); under
                                     SBE_CE_LAST_ONLY also a table-entry record that is not its entry's last */
#define SBE_CE_EMITTED 1u         /* the frame is out[out_off[i] .. out_off[i+1]) */
#define SBE_CE_HOST 2u            /* topic_idx[i] >= k (SBE_TOPIC_UNKNOWN, SBE_TOPIC_HOST) or topic_id of the
                                     entry is 0: the host resolves the topic, or owes the reference's JSON
                                     fallback (src/commit_manager.cpp:134-175), which
                                     sbe_emit_commit_offsets_ex builds on the device; 0 bytes */
#define SBE_CE_E109_MESSAGE_ID 3u /* messageId over 65534 bytes: computeLength throws [E109]; 0 bytes */
#define SBE_CE_OVERFLOW 4u        /* the frame ends past out_capacity: not written, and no byte of out from the
                                     end of the last frame that fits is touched */
#define SBE_CE_LAST_ONLY 0x1u     /* flag: emit only record plan->last[topic_idx[i]] of each table entry, at most
                                     k frames (the once-per-entry shortcut of a batch commit; no reference
                                     counterpart; SBE_EINVAL together with a mask).  SBE_CE_HOST records are
                                     reported as without the flag */

/* out_off / totals always describe the full layout, whatever out_capacity is (SBE_CE_OVERFLOW
 * records keep their length), so a call with out = NULL, out_capacity = 0 sizes a batch. */
typedef struct sbe_commit_emit_out {
    uint64_t* out_off;  /* [n + 1] record order; a record without a frame has length 0 */
    uint8_t* status;    /* [n] SBE_CE_* */
    uint64_t* emit_idx; /* [n] or NULL: the first totals[0] entries are written, the indices of the records
                           with a frame (EMITTED or OVERFLOW), ascending */
    uint64_t* totals;   /* [3] records with a frame, their bytes (= out_off[n]), SBE_CE_HOST records */
} sbe_commit_emit_out;

/* Bytes of device workspace for n records (frame lengths and block sums only, no text). */
size_t sbe_commit_emit_workspace_size(uint64_t n);
/* Upper bound of the frames of n emitting records whose messageIds and messageIdentifiers total
 * id_bytes (the ids lie inside the records: rec_off[n] - rec_off[0] bounds their part). */
uint64_t sbe_commit_emit_output_bound(uint64_t n, uint64_t id_bytes, int session);

/* in / rec_off / dec: the arguments and outputs of the decode call; plan: what sbe_classify_commits
 * wrote for them with a table of k entries (cm, topic_idx; last under SBE_CE_LAST_ONLY).
 * topic_id [k]: CommitManager::topic_to_id of entry j, 0 = unknown.  The identifier table is laid
 * out and clamped as the topic table is: entry j = ident_arena[ident_off[j] .. ident_off[j+1]),
 * ident_arena readable for SBE_COMMIT_TABLE_BYTES, offsets clamped to that, a reversed entry empty;
 * the host does not read ident_off.  mask: [n] u8 callback_ok, or NULL = all.
 * Alignment: u32 arrays 4 B, u64 arrays 8 B, workspace 16 B; out needs none.  n < 2^32.
 * n == 0 is SBE_OK with out_off[0] = 0 and totals zeroed (only res, out_off, totals, k, flags and
 * session are looked at).  SBE_EINVAL (nothing written): a null pointer where n > 0, k == 0 or
 * k > SBE_COMMIT_MAX_TOPICS, a misaligned array, unknown flag bits, SBE_CE_LAST_ONLY with a mask,
 * session not 0 / 1, out NULL with a capacity; SBE_ENOSPC: workspace too small.
 * On `stream`: the sizing launch, one scan launch over its block sums, the writing launch.  No atomics:
 * a repeated call writes identical results. */
int sbe_emit_commit_offsets(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const sbe_decoded* dec,
                            const sbe_commit_out* plan, const uint32_t* topic_id, const uint8_t* ident_arena,
                            const uint32_t* ident_off, uint32_t k, const uint8_t* mask, uint32_t flags,
                            int session, int64_t leadership_term_id, int64_t cluster_session_id, uint8_t* out,
                            uint64_t out_capacity, const sbe_commit_emit_out* res, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- the legacy COMMIT_OFFSET TopicMessage for topics without a numeric id ----
 * CommitManager::topic_to_id (src/commit_manager.cpp:16-22) knows four names; for every other
 * topic build_commit_offset_message takes its fallback (:134-175): a TopicMessage
 *   [the 32-B SessionMessageHeader when `session`]
 *   header {16,1,1,1}, u64 timestamp = now_ns, u64 sequenceNumber = 0, u16 + "_subscriptions",
 *   u16 + "COMMIT_OFFSET", u16 + uuid, u16 + text, u16 + "{}"
 * with uuid = "commit_offset_" + messageIdentifier + "_" + decimal clock (send_commit_offset passes
 * offset.message_identifier as client_id, src/cluster_client.cpp:678) and text = the jsoncpp object
 * written with indentation "" (keys sorted, no white space; also serialize_commit_offset :197-209):
 *   {"action":"COMMIT_OFFSET","messageIdentifier":Q,"message_id":Q,"sequence_number":D,
 *    "timestamp_nanos":D,"topic":Q}
 * Q = valueToQuotedStringN(.., emitUTF8 = false), D = unsigned decimal; message_id and
 * sequence_number as in the Lite frame, timestamp_nanos = dec->ts[i].
 * Two quirks of the reference are kept.  putUuid / putPayload take the length as std::uint16_t
 * (TopicMessage.h:865-879): a field of L bytes stores L mod 65536 and that many leading bytes.
 * The flyweight is wrapped with wrapForEncode(buf, 8, 1048 - 8) and its positions are absolute
 * (TopicMessage.h:210-219, 267-274), so with u and p the two stored lengths the record is
 * 63 + u + p bytes and the reference throws "buffer too short [E100]" exactly when that exceeds
 * 1040 (this path has no computeLength, hence no E109).
 *
 * With fb != NULL the status of record i is the first line that applies:
 *   1. SBE_CE_NONE as above.
 *   2. A table entry with topic_id != 0: the Lite frame as above (EMITTED, E109, OVERFLOW).
 *   3. A table entry with topic_id == 0: the JSON frame, topic = the entry's text in fb's topic
 *      table, messageIdentifier = the entry's identifier; under SBE_CE_LAST_ONLY only the entry's
 *      last record (the others SBE_CE_NONE).
 *   4. topic_idx == SBE_TOPIC_UNKNOWN and topic_kind == SBE_TOPIC_KIND_STRING: topic = the token
 *      plan->topic_off / topic_len (kept inside the record), messageIdentifier = default_ident; the
 *      Lite frame with id 1..4 when the token is one of topic_to_id's names, else the JSON frame.
 *      SBE_CE_LAST_ONLY does not filter these records.
 *   5. SBE_CE_HOST: SBE_TOPIC_HOST, and SBE_TOPIC_UNKNOWN with an escaped string. */
#define SBE_CE_EMITTED_JSON 5u  /* the JSON frame is out[out_off[i] .. out_off[i+1]) */
#define SBE_CE_E100_FALLBACK 6u /* 63 + u + p > 1040: the reference throws [E100]; 0 bytes */
#define SBE_CE_FALLBACK_REC_MAX 1040u

typedef struct sbe_commit_fallback {
    const uint8_t* topic_arena;   /* the classify call's topic table (device), clamped the same way */
    const uint32_t* topic_off;    /* [k + 1] */
    const uint8_t* default_ident; /* device; config_.client_id; readable for default_ident_len bytes */
    uint32_t default_ident_len;   /* <= SBE_COMMIT_TABLE_BYTES */
    uint64_t now_ns;              /* TopicMessage.timestamp of every JSON frame of the call */
    uint64_t uuid_ns;             /* record i's uuid ends in the decimal of uuid_ns + i */
} sbe_commit_fallback;

/* Upper bound of the frames of n records under a fallback: each at most the larger of its Lite
 * frame and SBE_CE_FALLBACK_REC_MAX + SBE_SESSION_HDR_LEN (id_bytes as for
 * sbe_commit_emit_output_bound). */
uint64_t sbe_commit_fallback_output_bound(uint64_t n, uint64_t id_bytes, int session);

/* sbe_emit_commit_offsets with the fallback fb; fb == NULL is sbe_emit_commit_offsets itself (the
 * same launches, the same results).  The reference reads the clock per record (twice: timestamp
 * and uuid); a batch has one reading, so every JSON frame carries now_ns and record i's uuid ends
 * in uuid_ns + i, which keeps the uuids of one call distinct and ascending.  That convention has
 * no reference counterpart.  out_off, emit_idx and totals keep their meaning: totals[0] counts
 * frames of either kind (EMITTED, EMITTED_JSON, OVERFLOW), totals[2] the SBE_CE_HOST records left.
 * Workspace: sbe_commit_emit_workspace_size(n), lengths and block sums, never text.
 * With fb, dec->ts, plan->topic_kind, plan->topic_off and plan->topic_len are read as well.
 * SBE_EINVAL as for sbe_emit_commit_offsets, and (whatever n is) a null member pointer of fb,
 * default_ident_len > SBE_COMMIT_TABLE_BYTES, a misaligned fb->topic_off; for n > 0 a null or
 * misaligned dec->ts / plan->topic_kind / topic_off / topic_len. */
int sbe_emit_commit_offsets_ex(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const sbe_decoded* dec,
                               const sbe_commit_out* plan, const uint32_t* topic_id, const uint8_t* ident_arena,
                               const uint32_t* ident_off, uint32_t k, const uint8_t* mask, uint32_t flags,
                               int session, int64_t leadership_term_id, int64_t cluster_session_id, uint8_t* out,
                               uint64_t out_capacity, const sbe_commit_emit_out* res, void* workspace,
                               size_t workspace_bytes, void* stream, const sbe_commit_fallback* fb);

/* ================================= ack correlation ================================= */
/* The step of the client's message loop that joins the two directions: publish_topic remembers
 * every offered record (remember_outgoing(uuid, ts), src/cluster_client.cpp:1860-1861, :1920-1922,
 * an emplace into std::unordered_map<std::string, std::uint64_t> inflight_,
 * include/aeron_cluster/cluster_client.hpp:420), and on_ack_default (:1924-1941) looks every ack's
 * message_id up there: found, it erases the entry and reports now - send_ns; not found, now -
 * ack.timestamp_nanos.  Here both run on whole batches against a hash table in caller-owned
 * device memory that lives across calls.
 *
 * The table: sbe_inflight_table_size(capacity) bytes, 64-B aligned; one 64-B header, then
 * `capacity` slots of 64 B; capacity a power of two, 64 .. 2^31.  The header's first words, for a
 * caller that reads them with its own copy:
 *   +0 u64 capacity   +8 u64 live (entries that can still match)
 *   +16 u64 used (slots that are not empty, erased ones included)   +24 u32 tag_bits
 *   +32 u64 answered (live entries a sbe_inflight_lookup_keys call has answered)
 * Limits: keys are stored inline, zero-padded, up to SBE_INFLIGHT_KEY_MAX bytes (the reference's
 * "pub_" + now_nanos() is at most 24); a longer key is reported, not stored (the host mirror keeps
 * those in a map of its own).  Erased slots are not reused by inserts: sbe_inflight_rehash into a
 * fresh table reclaims them.  A table serves one stream at a time; calls take effect in stream
 * order.  The header is device memory, which the host does not read: a null or misaligned table is
 * SBE_EINVAL, while a table whose header is not one sbe_inflight_init wrote is found on the device,
 * which then treats it as holding nothing and having no room (every remembered record SBE_INF_FULL,
 * no ack matched, a rehash copies nothing) and leaves it untouched. */
#define SBE_INFLIGHT_KEY_MAX 40u
/* status[i] of sbe_inflight_remember */
#define SBE_INF_INSERTED 0u     /* the record was stored */
#define SBE_INF_DUPLICATE 1u    /* the key was live already, or a smaller index of this call has it;
                                   the stored ts is unchanged (emplace) */
#define SBE_INF_SKIPPED 2u      /* mask[i] was 0: the offer failed (:1860) */
#define SBE_INF_KEY_TOO_LONG 3u /* over SBE_INFLIGHT_KEY_MAX bytes: not stored */
#define SBE_INF_FULL 4u         /* no free slot was found */
/* code[i] of sbe_inflight_match_acks */
#define SBE_ACK_NONE 0u      /* status is neither SBE_ST_EG_ACK_SIMPLE nor SBE_ST_EG_ACK: no ack callback */
#define SBE_ACK_MATCHED 1u   /* a non-empty id was found live; the entry is erased and `live` drops */
#define SBE_ACK_UNMATCHED 2u /* the id is empty (every simple ack) or was not found */
#define SBE_ACK_LONG_ID 3u   /* the id is over SBE_INFLIGHT_KEY_MAX bytes: it cannot be in the table */

/* 64 + 64 * capacity; 0 if capacity is not a power of two in 64 .. 2^31. */
size_t sbe_inflight_table_size(uint64_t capacity);

/* Make `table` (table_bytes >= sbe_inflight_table_size(capacity)) an empty table: a memset and a
 * one-wave launch on `stream`.  tag_bits (1..30, 0 = 30): the hash bits a slot keeps as a filter
 * in front of the comparison of the key bytes; results are the same for every value (1 makes every
 * probe of an occupied slot reach the byte comparison half of the time, 30 next to never).
 * SBE_EINVAL: null or misaligned table, bad capacity, table_bytes too small, tag_bits > 30. */
int sbe_inflight_init(void* table, size_t table_bytes, uint64_t capacity, uint32_t tag_bits, void* stream);

/* Workspace bytes of sbe_inflight_remember, sbe_inflight_match_acks, sbe_inflight_note_keys and
 * sbe_inflight_lookup_keys for n records (4-B aligned). */
size_t sbe_inflight_workspace_size(uint64_t n);

/* remember_outgoing for records 0 .. n-1, in order.  Key i is arena[key_off[i*stride] ..) with
 * key_len[i*stride] bytes (str_off + 2, str_len + 2, stride 5: the uuid column of an sbe_tm_batch
 * with explicit offsets); ts[i] is the send time, 0 or ts == NULL: ts_default (the encoders' rule,
 * so the same arrays serve both); mask: NULL or u8[n], 0 = the offer failed, the record is
 * skipped.  emplace semantics: the first record of a key wins, against the table's live entries
 * and against smaller indices of the same call.  An empty key is stored like any other.
 * status: [n] u8 or NULL.  With used + n < capacity no record is SBE_INF_FULL and every status and
 * the table's content are those of the sequential loop (it is enough that used + the number of
 * distinct new keys of the call stays below capacity).  Otherwise which records are SBE_INF_FULL
 * is unspecified, but every record gets exactly one status, exactly the SBE_INF_INSERTED ones were
 * added, and after a call that reported SBE_INF_FULL used == capacity.
 * Two launches on `stream`.  SBE_EINVAL (before any launch): a null table / arena / key_off /
 * key_len / workspace, stride 0, n >= 2^32, table not 64-B, ts not 8-B, key_off / key_len /
 * workspace not 4-B aligned; SBE_ENOSPC: workspace too small.  n == 0 is SBE_OK. */
int sbe_inflight_remember(void* table, const uint8_t* arena, const uint32_t* key_off, const uint32_t* key_len,
                          uint32_t stride, const uint64_t* ts, uint64_t ts_default, const uint8_t* mask,
                          uint64_t n, uint8_t* status, void* workspace, size_t workspace_bytes, void* stream);

typedef struct sbe_ack_out {
    uint8_t* code;     /* [n] SBE_ACK_* */
    uint64_t* base_ns; /* [n] what on_ack_default subtracts from now_nanos(): the remembered send time
                          (MATCHED) or the ack's timestamp_nanos (otherwise); 0 for SBE_ACK_NONE */
    uint64_t* counts;  /* [2] {matched, acks not matched (UNMATCHED + LONG_ID)}, set by the call
                          itself; or NULL */
} sbe_ack_out;

/* on_ack_default for a batch decoded with sbe_decode_batch(SBE_DEC_ON_EGRESS) on the same in /
 * rec_off (dec: its status, ts, view_off, view_len), in record order; the id is view 0 of a full
 * ack.  Erase-on-match is sequential: of several acks of one call with the same id only the
 * smallest index matches, the others are SBE_ACK_UNMATCHED (the first one erased the entry).
 * A memset of counts and two launches on `stream`.  SBE_EINVAL as for sbe_inflight_remember (out,
 * code, base_ns, in, rec_off, dec and its four arrays must not be null; rec_off / ts / base_ns /
 * counts 8-B, view arrays 4-B aligned).  n == 0 is SBE_OK with counts = {0, 0}: only table, out
 * and counts are looked at. */
int sbe_inflight_match_acks(void* table, const uint8_t* in, const uint64_t* rec_off, uint64_t n,
                            const sbe_decoded* dec, const sbe_ack_out* out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Copy the live entries of src, each with its ts, into dst, an initialised empty table of any
 * capacity with room: the caller checks live(src) < capacity(dst) from the header words (entries
 * that find no slot are dropped).  src is unchanged; used(dst) == live(src) afterwards.  One launch
 * on `stream`.  SBE_EINVAL: null, misaligned or identical tables. */
int sbe_inflight_rehash(const void* src, void* dst, void* stream);

/* ================================ delivery tracking ================================ */
/* What the subscriber's callback keeps per delivered record
 * (examples/pubsub_reconnect_test.cpp:625-691, the same code again from :1190), on the tables of
 * the section above: which message ids and client order ids were seen before and how often, and
 * which sent order a delivery answers.  The example's sets are never evicted, so the results are
 * exactly those of the sequential callback.
 *
 * Keys are byte ranges anywhere in one device buffer: key i is buf[key_pos[i] .. key_pos[i] +
 * key_len[i]) (key_pos: device u64 [n], 8-B aligned; key_len: device u32 [n], 4-B aligned;
 * SBE_NO_KEY: the record has no key).  A range is clamped into [0, buf_bytes) before a byte of it
 * is read: key_pos to at most buf_bytes, then key_len to what is left (so a key_pos at or past
 * buf_bytes is the empty key).  A zero-length key is a key, as for sbe_inflight_remember.
 * sbe_inflight_workspace_size(n) also sizes the workspace of both calls.  Each result depends on
 * the table before the call and on the record order only. */
#define SBE_NO_KEY 0xFFFFFFFFu
/* code[i] of sbe_inflight_note_keys */
#define SBE_DLV_NONE 0u  /* no key: nothing is looked up */
#define SBE_DLV_NEW 1u   /* the key was not live and no smaller index of this call has it: it is stored */
#define SBE_DLV_AGAIN 2u /* the key was live, or a smaller index of this call has it */
#define SBE_DLV_LONG 3u  /* over SBE_INFLIGHT_KEY_MAX bytes (after the clamp): not stored */
#define SBE_DLV_FULL 4u  /* no free slot was found */
/* code[i] of sbe_inflight_lookup_keys */
#define SBE_SENT_NONE 0u    /* no key */
#define SBE_SENT_UNKNOWN 1u /* the key is not live */
#define SBE_SENT_FIRST 2u   /* live, not yet answered, and the smallest index of the call that has it:
                               value[i] is the stored value; the entry becomes answered and stays live */
#define SBE_SENT_REPEAT 3u  /* live, and answered before the call or a smaller index of the call has it */
#define SBE_SENT_LONG 4u    /* over SBE_INFLIGHT_KEY_MAX bytes: it cannot be in the table */

/* Test-and-insert that counts.  The 8-byte value of a slot holds the number of deliveries of its
 * key: every record that is NEW or AGAIN adds one (a key stored by sbe_inflight_remember counts on
 * from its send time).  code: [n] u8 SBE_DLV_*.  count: [n] u32, for NEW and AGAIN the low 32 bits
 * of (the key's value after the whole call) - 1, i.e. what record_duplicate_delivery returned for
 * the last redelivery of that id in the call; 0 for every other code.  totals: NULL or device
 * u64 [2] {NEW, AGAIN}, zeroed by the call (8-B aligned).  With used + the distinct new keys of the
 * call below capacity no record is SBE_DLV_FULL.  header +8 live and +16 used grow by the NEW
 * records.  A memset of totals and two launches on `stream`.  SBE_EINVAL (before any launch): a
 * null table / buf / key_pos / key_len / code / count / workspace, n >= 2^32, table not 64-B,
 * key_pos / totals not 8-B, key_len / count / workspace not 4-B aligned; SBE_ENOSPC: workspace too
 * small.  n == 0 is SBE_OK with totals zeroed: only table and totals are looked at. */
int sbe_inflight_note_keys(void* table, const uint8_t* buf, uint64_t buf_bytes, const uint64_t* key_pos,
                           const uint32_t* key_len, uint64_t n, uint8_t* code, uint32_t* count, uint64_t* totals,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Lookup that marks on first sight.  "Answered" is state of a live entry (bit 0 of its slot word;
 * header +32 u64 answered counts such entries): sbe_inflight_remember still reports the key as
 * SBE_INF_DUPLICATE and leaves it answered, sbe_inflight_match_acks still matches and erases it
 * (answered drops), sbe_inflight_rehash carries it over.  code: [n] u8 SBE_SENT_*.  value: [n] u64,
 * the stored value for FIRST, 0 otherwise (8-B aligned).  totals: NULL or device u64 [3]
 * {FIRST, REPEAT, UNKNOWN + LONG}, zeroed by the call.  Launches, errors and n == 0 as for
 * sbe_inflight_note_keys (value in the place of count). */
int sbe_inflight_lookup_keys(void* table, const uint8_t* buf, uint64_t buf_bytes, const uint64_t* key_pos,
                             const uint32_t* key_len, uint64_t n, uint8_t* code, uint64_t* value, uint64_t* totals,
                             void* workspace, size_t workspace_bytes, void* stream);

/* clear_duplicate_tracking (:70-73) for a table of sbe_inflight_note_keys: the value of every live
 * entry goes back to 1, one delivery and no redelivery, so every count is 0 again and the next
 * redelivery of an id reports 1, as record_duplicate_delivery does after the example cleared its
 * counters (a value of 0 would leave every id seen before the call one short for ever after).
 * Membership and the answered state stay.  One launch.  SBE_EINVAL: null or misaligned table. */
int sbe_inflight_reset_values(void* table, void* stream);

/* The paths sbe_delivery_keys expects `ids` to have been extracted over (view 3), in this order:
 *   0 message                         1 message.message
 *   2 message.message.client_order_id 3 message.message.order_id
 *   4 message.message.order_details   5 message.message.order_details.client_order_id
 *   6 message.order_details           7 message.order_details.client_order_id
 *   8 uuid */
#define SBE_DLV_PATHS 9u

typedef struct sbe_delivery_key_out { /* device arrays of n elements; u64 8-B, u32 4-B aligned */
    uint64_t* msg_pos;  /* rec_off[i] + view 2 (message_id), clamped into the record */
    uint32_t* msg_len;  /* SBE_NO_KEY: not selected, or an empty id (:628) */
    uint64_t* coid_pos; /* the client_order_id: rec_off[i] + the member's range, clamped into the record */
    uint32_t* coid_len; /* SBE_NO_KEY: no string was found, or an empty one (:648, :669) */
    uint8_t* coid_kind; /* SBE_JX_STRING, SBE_JX_STRING_ESC (the raw range: the host decodes it before
                           it can be compared) or SBE_JX_MISSING */
    uint64_t* oid_pos;  /* the order_id, likewise */
    uint32_t* oid_len;
    uint8_t* oid_kind;
    uint8_t* selected;  /* 1: the callback's outer if (:578) holds: SBE_ST_TM and select[i] */
    uint64_t* totals;   /* [2] {selected records, ids of kind SBE_JX_STRING_ESC}, zeroed by the call */
} sbe_delivery_key_out;

/* The keys of a decoded batch: dec is a parse-mode decode of rec_off's records, ids an
 * sbe_json_extract_batch(view 3) of them over the SBE_DLV_PATHS paths, select NULL (every
 * TopicMessage) or a device u8 [n].  Positions are offsets into the buffer rec_off indexes, ready
 * for the two calls above.  The ids follow the callback (:592-619): the document must be
 * SBE_JX_OK and its root an object; message.message an object: client = string 2, order =
 * string 3, and an empty client falls through to string 5 when 4 is an object; otherwise
 * message.order_details (6) an object: client = string 7; an empty order is replaced by a
 * non-empty string 8.  Only strings count.  A non-empty SBE_JX_STRING_ESC decodes to a non-empty
 * string and stops a fall-through.  The kind is that of the member the rule ended on (an empty
 * string keeps SBE_JX_STRING with length SBE_NO_KEY); a position whose length is SBE_NO_KEY is
 * rec_off[i].  One launch after a memset of totals; every element i < n of the nine arrays is
 * written.  n == 0 is SBE_OK with totals zeroed.  SBE_EINVAL: a null pointer (select excepted),
 * n >= 2^32, an array below its alignment. */
int sbe_delivery_keys(const uint64_t* rec_off, uint64_t n, const sbe_decoded* dec, const uint8_t* select,
                      const sbe_json_out* ids, const sbe_delivery_key_out* out, void* stream);

/* ============================== message kinds, order select ============================== */
/* The test in front of all of the above, the first line of the callback (:578-579):
 *   result.is_order_message() || (result.is_topic_message() && result.message_type == "CREATE_ORDER")
 * i.e. the ParseResult predicates (include/aeron_cluster/sbe_messages.hpp:332-406) of every record of
 * a parse-mode decode, and classify_topic (include/aeron_cluster/topic_router.hpp) of its topic.
 * pred[i] is a set of: */
#define SBE_PR_SESSION_EVENT 0x1u  /* is_session_event(): template 2, schema 111 */
#define SBE_PR_TOPIC_MESSAGE 0x2u  /* is_topic_message(): template 1 and schema 1 or 111; template 2 and schema 1;
                                      or a message type that contains "ORDER" or "TopicMessage" */
#define SBE_PR_ACKNOWLEDGMENT 0x4u /* is_acknowledgment(): template 2, schema 1 */
#define SBE_PR_ORDER_MESSAGE 0x8u  /* is_order_message(): is_topic_message() and a type that contains "ORDER", or
                                      a payload that contains order_details, token_pair, quantity, side or
                                      client_order_id */
/* topic_class[i]: classify_topic of view 0 of an SBE_ST_TM record (0 for any other record) */
#define SBE_TC_UNKNOWN 0u
#define SBE_TC_ORDERS 1u  /* "orders", "order_request_topic" */
#define SBE_TC_CONTROL 2u /* "_subscriptions", "_ack", "_control", "_internal" */

typedef struct sbe_select_out { /* device arrays */
    uint8_t* pred;        /* [n] SBE_PR_* */
    uint8_t* select;      /* [n] or NULL: 1 for an SBE_ST_TM record with SBE_PR_ORDER_MESSAGE (the callback's test
                             for the records sbe_json_extract_batch and sbe_delivery_keys serve; its CREATE_ORDER
                             clause is implied by the "ORDER" search), else 0 */
    uint8_t* topic_class; /* [n] or NULL: SBE_TC_* */
    uint64_t* totals;     /* [2] {records with select 1, records with SBE_PR_ORDER_MESSAGE}, zeroed by the call
                             (8-B aligned) */
} sbe_select_out;

/* The predicates are those of the ParseResult the record decodes to: an SBE_ST_TM has message type
 * view 1 and payload view 3; an SBE_ST_ACK the type "Acknowledgment" and payload view 1 ("SUCCESS"
 * under SBE_FL_PAYLOAD_DEFAULT), and being template 2 / schema 1 it is a topic message to the
 * reference, so an Ack whose payload contains "side" has SBE_PR_ORDER_MESSAGE (select stays 0); an
 * SBE_ST_SESSION_EVENT the type "SessionEvent" and payload view 3; an error status has no strings and
 * an all-zero header (SBE_ST_ERR_UNKNOWN_TYPE keeps hdr); a status the parse mode does not produce
 * gives pred 0.  Matching is on bytes, case-sensitive, and a match lies wholly inside its view; views
 * are kept inside their records whatever the descriptors say.  in / rec_off / dec: the arguments and
 * outputs of the decode call; dec->status, flags, hdr, view_off and view_len are read (ts and seq may
 * be null).  One launch after a memset of totals, no workspace; every element i < n of each non-null
 * array is written and nothing else.  n == 0 is SBE_OK with totals zeroed: only out and out->totals
 * are looked at.  SBE_EINVAL (before any launch, nothing written): a null pointer (select and
 * topic_class excepted), n >= 2^32, rec_off or totals not 8-byte, hdr not 2-byte or a view array not
 * 4-byte aligned. */
int sbe_order_select(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const sbe_decoded* dec,
                     const sbe_select_out* out, void* stream);
/* Bytes of the kernel's LDS window (a multiple of 16): a payload that crosses it is searched in
 * overlapping rounds.  For callers and tests that want records on either side of that edge. */
uint32_t sbe_order_select_window(void);

/* ================================ delivery reports ================================ */
/* The read side of the tables above: what examples/pubsub_reconnect_test.cpp prints from its sets
 * (printMessageComparison :130-204, printClientOrderAudit :206-274, printLatencyReport :276-353)
 * without copying a table back.  No call here modifies a table. */
#define SBE_LIST_MAX 64u
#define SBE_LIST_IN_OTHER 0x1u     /* keep keys that are live in `other` */
#define SBE_LIST_NOT_IN_OTHER 0x2u /* keep keys that are not live in `other` */
#define SBE_LIST_ANSWERED 0x4u     /* keep entries with the answered bit */
#define SBE_LIST_UNANSWERED 0x8u   /* keep entries without it */
typedef struct sbe_key_list_out { /* device arrays */
    uint64_t* count;   /* [1] every LIVE entry that passes the filter, listed or not (8-B aligned) */
    uint8_t* key;      /* [limit][SBE_INFLIGHT_KEY_MAX] zero-padded key bytes */
    uint32_t* len;     /* [limit] (4-B aligned) */
    uint64_t* value;   /* [limit] the slot's 8-byte value (8-B aligned) */
    uint8_t* answered; /* [limit] 0 / 1 */
} sbe_key_list_out;

/* Workspace bytes of sbe_inflight_list_keys for `limit` rows; 0 for a limit over SBE_LIST_MAX.
 * It does not depend on the capacity of a table. */
size_t sbe_inflight_list_workspace_size(uint32_t limit);

/* The entries of `table` that pass a filter, smallest keys first.  A LIVE entry passes when the
 * membership test in `other` holds (SBE_LIST_IN_OTHER / SBE_LIST_NOT_IN_OTHER: exactly one of them
 * with a table `other`, none without), the answered test holds (SBE_LIST_ANSWERED /
 * SBE_LIST_UNANSWERED, at most one) and its value is >= min_value (0: every value; 2 on a table of
 * message ids: the ids delivered more than once).  A key is a member of `other` when a LIVE slot of
 * its chain there holds it (an erased key is not); `other` may have another capacity and other
 * tag_bits.  count[0] is the number of passing entries.  Rows j < min(count, limit) hold the
 * min(count, limit) smallest passing keys ascending in std::string::compare order (bytes as
 * unsigned, a proper prefix before the longer key: the 40 zero-padded bytes, then len); rows at or
 * past that are not written.  limit == 0 only counts: the row arrays may be null.  A table without
 * a valid header holds nothing: count 0 as `table`, no member as `other`.  Two launches on `stream`.
 * SBE_EINVAL (before any launch, nothing written): a null table / out / count / workspace, a null
 * row array with limit > 0, limit > SBE_LIST_MAX, an unknown flag bit, both bits of a pair, a
 * membership bit without `other` or `other` without one, other == table, a table not 64-B, count /
 * value not 8-B or len not 4-B aligned; SBE_ENOSPC: workspace too small. */
int sbe_inflight_list_keys(const void* table, const void* other, uint32_t flags, uint64_t min_value, uint32_t limit,
                           const sbe_key_list_out* out, void* workspace, size_t workspace_bytes, void* stream);

/* The latency log: caller-owned device memory that lives across calls, 64-B aligned:
 *   +0 u64 capacity   +8 u64 count   +16 u64 dropped   +24 u32 magic       (64-B header)
 *   +64 int64 lat[capacity], then u64 tag[capacity]
 * sbe_latency_log_size: 64 + 16 * capacity bytes for a capacity in 1 .. 2^31, 0 for any other.
 * A log without a valid header is full and empty: nothing is appended, a report sees count 0. */
size_t sbe_latency_log_size(uint64_t capacity);

/* Make `log` (log_bytes >= sbe_latency_log_size(capacity)) an empty log.  One launch.  SBE_EINVAL:
 * null or misaligned log, bad capacity, log_bytes too small. */
int sbe_latency_log_init(void* log, size_t log_bytes, uint64_t capacity, void* stream);

/* Workspace bytes of sbe_latency_append for n records (8-B aligned). */
size_t sbe_latency_append_workspace_size(uint64_t n);

/* The samples of one sbe_inflight_lookup_keys call (its code / value outputs, n records): every i
 * with code[i] == SBE_SENT_FIRST, in index order, appends at the log's cursor
 *   lat = (int64)(now_ns - value[i]) / (int64)unit_ns     (the difference mod 2^64, then C++
 *                                                          division: truncation toward zero)
 *   tag = tag_base + i                                    (mod 2^64)
 * unit_ns 1000000 is the example's duration_cast<milliseconds>.  Samples are placed by a scan over
 * the records, so the log is a function of the call sequence.  Samples that do not fit are dropped
 * and counted in the header's `dropped`; count never exceeds capacity.  Three launches on `stream`.
 * SBE_EINVAL (before any launch): a null or misaligned log, n >= 2^32, and for n > 0 a null code /
 * value / workspace, value or workspace not 8-B aligned, unit_ns outside 1 .. 2^62; SBE_ENOSPC:
 * workspace too small.  n == 0 is SBE_OK: only log is looked at. */
int sbe_latency_append(void* log, const uint8_t* code, const uint64_t* value, uint64_t n, uint64_t now_ns,
                       uint64_t unit_ns, uint64_t tag_base, void* workspace, size_t workspace_bytes, void* stream);

#define SBE_LAT_MAX_PCT 16u
typedef struct sbe_latency_report_out { /* device arrays; 8-B aligned, order 4-B */
    uint64_t* count;     /* [1] samples in the log */
    int64_t* stats;      /* [3] sum (mod 2^64), min, max; all 0 when count == 0 */
    int64_t* pct_value;  /* [n_pct]; 0 when count == 0 */
    uint64_t* pct_index; /* [n_pct] the index the value was read from; 0 when count == 0 */
    int64_t* sorted;     /* NULL, or [log capacity]: the first `count` entries written, ascending */
    uint32_t* order;     /* NULL, or [log capacity]: order[j] = log position of sorted[j] */
} sbe_latency_report_out;

/* Workspace bytes of sbe_latency_report for a log of `capacity` samples; 0 for a bad capacity. */
size_t sbe_latency_report_workspace_size(uint64_t capacity);

/* printLatencyReport's numbers.  The samples are ordered ascending by (lat, log position): a
 * stable sort of signed 64-bit values (the example's descending row list is `order` read from the
 * end).  For pct[p] the index is computed in double precision on the device from the log's count,
 * with the example's operations in its order (:322-326):
 *   rank = (pct / 100.0) * (double)count;  idx = rank <= 0.0 ? 0 : (size_t)ceil(rank) - 1;
 *   idx = min(idx, count - 1)
 * which is not the textbook index: with 1000 samples p99.9 reads index 999.  The average is
 * (double)sum / (double)count on the host, as :334.  pct is host memory, read during the call.
 * The log is not modified.  The host cannot read the log's capacity: a workspace of
 * sbe_latency_report_workspace_size(capacity) bytes always suffices, and a log holding more samples
 * than workspace_bytes provides for is reported like a log without a valid header (count 0).  A
 * memset of stats and 25 launches on `stream` (8 passes of histogram, scan, scatter; one to read
 * the results).  SBE_EINVAL (before any launch): a null log / out / count / stats / workspace,
 * n_pct > SBE_LAT_MAX_PCT, n_pct > 0 with a null pct / pct_value / pct_index, a pct that is not
 * finite or outside [0, 100], a log not 64-B or an array below its alignment; SBE_ENOSPC: a
 * workspace below sbe_latency_report_workspace_size(1). */
int sbe_latency_report(const void* log, const double* pct, uint32_t n_pct, const sbe_latency_report_out* out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ============================ Aeron fragment reassembly ============================ */
/* Replaces LocalFragmentReassembler::onFragment (src/cluster_client.cpp:39-82) for a batch of
 * fragments, in arrival order:
 *   flags[i] & (BEGIN|END) == BEGIN|END   the fragment is a whole message;
 *   otherwise   BEGIN clears the accumulator, the fragment is appended, END delivers the
 *               accumulator as one message and clears it.
 * in[frag_off[i] .. frag_off[i+1]) is fragment i (frag_off: n + 1 device u64).
 * Outputs: the delivered messages back to back in delivery order, out[msg_off[j] .. msg_off[j+1])
 * for j < m; then the open accumulator ("carry", bytes of a message whose END has not arrived)
 * at out[msg_off[m] .. msg_off[m] + carry).  counts (device u64[2]) = {m, carry}.  To continue
 * with the next batch, pass the carry bytes as its first fragment with flags 0 (a middle
 * fragment appends exactly as the accumulator would).
 * out must hold frag_off[n] - frag_off[0] bytes, msg_off n + 1 entries (entries past m, and the
 * bytes of out past the carry, are unspecified).  Alignment: frag_off / msg_off / counts 8 B; in,
 * flags and out need none.  Workspace: sbe_reassemble_workspace_size(n) bytes. */
#define SBE_FRAG_BEGIN 0x80u
#define SBE_FRAG_END 0x40u
size_t sbe_reassemble_workspace_size(uint64_t n);
int sbe_reassemble_fragments(const uint8_t* in, const uint64_t* frag_off, const uint8_t* flags, uint64_t n,
                             uint8_t* out, uint64_t* msg_off, uint64_t* counts, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ============================ Aeron term-buffer framing ============================ */
/* The step in front of sbe_reassemble_fragments: the walk a poll of one image does over a raw block
 * of a term buffer (Aeron's TermReader::read loop), which finds the fragments.  The frame layer is
 * third-party Aeron, which the reference tree does not carry: the semantics are restated here from
 * the data-frame layout, not pinned to a reference source.  A frame starts on a 32-byte boundary
 * with a 32-byte little-endian header:
 *   [0] i32 frame_length (header + payload, without alignment padding; <= 0: not yet committed)
 *   [4] i8 version  [5] u8 flags (SBE_FRAG_BEGIN / SBE_FRAG_END)  [6] u16 type (0: padding frame)
 *   [8] i32 term_offset  [12] i32 session_id  [16] i32 stream_id  [20] i32 term_id  [24] i64 reserved
 * and the next frame starts align(frame_length, 32) bytes on.  The walk:
 *   offset = start; fragments = 0
 *   while fragments < limit and offset < block_bytes:
 *       L = frame_length at offset
 *       L <= 0: stop UNCOMMITTED.  L < 32: stop SHORT.  offset + align(L, 32) > block_bytes: stop PARTIAL
 *       (the last two are this library's: it never reads outside the block whatever the bytes say)
 *       offset += align(L, 32); a frame whose type is not 0 is delivered: payload = the L - 32 bytes
 *       after its header, flags = its byte 5, fragments += 1 (a padding frame is consumed uncounted)
 *   stop LIMIT when fragments == limit, else END
 * with limit = min(fragment_limit, frag_capacity).  A frame that stops the walk is not consumed.
 * Payload bytes that look like headers are never frames: only the chain from `start` counts.
 * Outputs (device memory): the payloads back to back in delivery order in out (block_bytes - start
 * bytes are always enough; NULL: tables only), fragment i at out[frag_off[i] .. frag_off[i+1]),
 * frag_off[0] = 0, flags[i], frag_src[i] = the offset of its frame header in block (or NULL);
 * counts = {fragments, next (the offset the walk stopped at), payload bytes, SBE_TERM_STOP_*}.
 * out / frag_off / flags / counts[0] are the in / frag_off / flags / n of sbe_reassemble_fragments.
 * SBE_EINVAL (before anything touches a device): null o / counts / frag_off / flags; block_bytes or
 * start not a multiple of 32; start > block_bytes; block_bytes > 2^30; block not 16-B, frag_off /
 * counts not 8-B, frag_src not 4-B aligned; null block or workspace when block_bytes > start.
 * SBE_ENOSPC: block_bytes > start and workspace_bytes < sbe_term_scan_workspace_size(block_bytes).
 * block_bytes == start or limit == 0: one launch that writes counts and frag_off[0]; otherwise
 * three launches on `stream`. */
#define SBE_TERM_STOP_END 0u
#define SBE_TERM_STOP_LIMIT 1u
#define SBE_TERM_STOP_UNCOMMITTED 2u
#define SBE_TERM_STOP_SHORT 3u
#define SBE_TERM_STOP_PARTIAL 4u
typedef struct sbe_term_out {
    uint64_t* frag_off; /* [frag_capacity + 1] offsets of the compacted payloads in `out` */
    uint8_t* flags;     /* [frag_capacity] header byte 5 of each delivered frame */
    uint32_t* frag_src; /* [frag_capacity] or NULL: offset of each delivered frame's header in block */
    uint64_t* counts;   /* [4] fragments, next, payload bytes, stop reason */
} sbe_term_out;
size_t sbe_term_scan_workspace_size(uint64_t block_bytes);
/* bytes of block one workgroup chains in LDS (a multiple of 32) */
uint32_t sbe_term_scan_tile(void);
int sbe_term_scan(const uint8_t* block, uint64_t block_bytes, uint64_t start, uint64_t fragment_limit,
                  uint64_t frag_capacity, uint8_t* out, const sbe_term_out* o, void* workspace,
                  size_t workspace_bytes, void* stream);

/* sbe_term_scan and sbe_reassemble_fragments as one call: a raw block and the open accumulator of
 * the calls before it in, whole messages out.  The fragment count stays in device memory (no host
 * read between the walk and the reassembly) and each payload byte is copied once, from the block or
 * the carry buffer straight into its message.
 * Walk: exactly sbe_term_scan's, with limit = min(fragment_limit, frag_capacity), the same five stop
 * reasons and the same rule for padding frames around the limit; counts[0..3] are what sbe_term_scan
 * writes for the same block, start, limit and capacity.  The carry is no fragment of the walk: it
 * does not count against the limit, is not in counts[0] or counts[2] and does not move `next`.
 * Reassembly: exactly sbe_reassemble_fragments over the delivered fragments in delivery order; with
 * carry_bytes > 0, one leading fragment with flags 0 that holds carry[0 .. carry_bytes) comes first.
 * So a first fragment with BEGIN drops the carry; a first fragment that is a BEGIN|END single is
 * delivered and the carry stays open; a first fragment with END delivers carry + fragment as one
 * message; with no fragment delivered (limit 0, start == block_bytes, an immediate stop) m = 0 and
 * the carry goes out unchanged.
 * Outputs (device memory): the messages back to back from out[0], message j at out[msg_off[j] ..
 * msg_off[j+1]) for j < m, msg_off[0] = 0; the open accumulator at out[msg_off[m] .. msg_off[m] +
 * counts[5]); counts = {fragments, next, payload bytes, SBE_TERM_STOP_*, messages m, carry bytes}.
 * Entries of msg_off past m and bytes of out past the carry are unspecified; nothing is written at
 * or past out[carry_bytes + block_bytes - start].  m <= fragments, so frag_capacity + 1 offsets are
 * enough.  To continue, pass the accumulator as the next call's carry: it may be a view of this
 * call's out, and the next call then writes to a second buffer (carry and out must not overlap).
 * SBE_EINVAL (before anything touches a device): everything sbe_term_scan refuses (block_bytes or
 * start not a multiple of 32; start > block_bytes; block_bytes > 2^30; block not 16-B aligned; null
 * block or workspace when block_bytes > start); null o / msg_off / counts / out; null carry with
 * carry_bytes > 0; msg_off or counts not 8-B aligned; carry_bytes + block_bytes - start > 2^31;
 * [carry, carry + carry_bytes) overlapping [out, out + out_capacity).  SBE_ENOSPC: out_capacity <
 * carry_bytes + block_bytes - start; block_bytes > start and workspace_bytes <
 * sbe_term_poll_workspace_size(block_bytes, frag_capacity).  A bad argument wins over a short buffer.
 * Every launch is enqueued on `stream`; the call does not wait, copy to the host or allocate.
 * block_bytes == start or limit == 0: one launch that writes counts and msg_off[0], and one that
 * copies the carry when there is one; otherwise seven launches (three of the walk, three of the
 * scan, the gather), and one more in front that enters the carry into the tables. */
typedef struct sbe_term_poll_out {
    uint64_t* msg_off;  /* [frag_capacity + 1]; message j = out[msg_off[j] .. msg_off[j+1]) for j < m */
    uint64_t* counts;   /* [6] fragments, next, payload bytes, SBE_TERM_STOP_*, messages m, carry bytes */
} sbe_term_poll_out;
size_t sbe_term_poll_workspace_size(uint64_t block_bytes, uint64_t frag_capacity);
int sbe_term_poll(const uint8_t* block, uint64_t block_bytes, uint64_t start, uint64_t fragment_limit,
                  uint64_t frag_capacity, const uint8_t* carry, uint64_t carry_bytes,
                  uint8_t* out, uint64_t out_capacity, const sbe_term_poll_out* o,
                  void* workspace, size_t workspace_bytes, void* stream);

/* The publish side, the mirror of sbe_term_scan: a batch of encoded records (`in`, rec_off[n + 1], as
 * sbe_encode_session_batch, sbe_publish_orders_batch and sbe_emit_commit_offsets leave them) appended
 * to a term-buffer block with Aeron's framing, as ExclusivePublication::offer ->
 * ExclusiveTermAppender::appendUnfragmentedMessage / appendFragmentedMessage /
 * handleEndOfLogCondition would one record at a time.  Third-party Aeron again: restated from the
 * data-frame layout above, not pinned to a reference source.  With maxp = mtu - 32 and
 *   required(L) = L <= maxp ? align(32 + L, 32)
 *                           : (L / maxp) * mtu + (L % maxp ? align(32 + L % maxp, 32) : 0)
 * the call is
 *   tail = start; appended = 0
 *   for i in 0..n:
 *       L = rec_off[i+1] - rec_off[i]
 *       rec_off[i+1] < rec_off[i] or rec_off[i+1] > in_bytes: stop BAD_RECORD
 *       (this library's own: it never reads outside `in`, whatever the offsets say)
 *       tail >= limit: stop LIMIT (offer's position < limit test: BACK_PRESSURED)
 *       L > max_message_length: stop TOO_LONG (checkMaxMessageLength; after the limit, as offer does)
 *       tail + required(L) > block_bytes:
 *           if tail < block_bytes: a padding-frame header at tail (frame_length = block_bytes - tail,
 *           type 0, flags 0xC0, the other fields as a data frame's); tail = block_bytes; stop TRIPPED
 *           (an exact fit is not a trip; at tail == block_bytes nothing is written)
 *       the frames of record i at tail; tail += required(L); appended += 1
 *   stop END when all n went in
 * A record that stops the call is not consumed: the caller goes on with records[appended:], into the
 * next term after TRIPPED.  Frames of one record: L <= maxp: one frame, flags 0xC0 (L == 0: 32
 * bytes); otherwise L / maxp full frames and one for the remainder if there is one, BEGIN (0x80) on the
 * first, END (0x40) on the last (the last full frame when L % maxp == 0), 0 in between.  Every data-
 * frame header: frame_length = 32 + payload bytes, hdr->version, the flags, type 1, term_offset =
 * hdr->term_offset_base + the frame's offset in block (the block may be a part of a term),
 * hdr->session_id / stream_id / term_id, reserved value 0.
 * The call writes every byte of [start, tail of the last appended record): headers, payloads and
 * zeros in each frame's alignment tail (Aeron leaves those to the pre-zeroed term; writing them makes
 * the block's content a function of the inputs); of a padding frame the 32 header bytes only, as Aeron
 * does; nothing else in the block and nothing outside it.  There is no ordering between frames (Aeron
 * commits a frame by writing its length last): this is a batch, not a concurrent publication, and the
 * block is complete when the call's work on `stream` is.  `in` and block must not overlap (not checked).
 * Outputs (device memory): counts = {appended, next (the tail), payload bytes appended,
 * SBE_TERM_APPEND_*}; rec_tail[i] (or NULL) = the block offset behind record i, what offer returns
 * for it, i < appended (the other elements are written with unspecified values).
 * SBE_EINVAL (before anything touches a device): null hdr / o / counts; null rec_off / in / block /
 * workspace when n > 0; block_bytes or start not a multiple of 32; start > block_bytes; block_bytes >
 * 2^30; mtu not a multiple of 32 or outside [64, 65504]; max_message_length > 2^30; block not 16-B,
 * rec_off / rec_tail / counts not 8-B aligned; n >= 2^32.  SBE_ENOSPC: n > 0 and workspace_bytes <
 * sbe_term_append_workspace_size(n).  n == 0: one launch that writes counts (END); otherwise four
 * launches on `stream` (three when start == block_bytes). */
#define SBE_TERM_APPEND_END 0u
#define SBE_TERM_APPEND_LIMIT 1u
#define SBE_TERM_APPEND_TRIPPED 2u
#define SBE_TERM_APPEND_TOO_LONG 3u
#define SBE_TERM_APPEND_BAD_RECORD 4u
typedef struct sbe_term_header {
    int32_t session_id;
    int32_t stream_id;
    int32_t term_id;
    int32_t term_offset_base; /* term offset of block[0] */
    uint8_t version;
} sbe_term_header;
typedef struct sbe_term_append_out {
    uint64_t* rec_tail; /* [n] or NULL: block offset behind record i, i < appended; the rest unspecified */
    uint64_t* counts;   /* [4] appended, next (tail), payload bytes appended, SBE_TERM_APPEND_* */
} sbe_term_append_out;
/* required(L): bytes of block the frames of an L-byte record take; host only, 0 on a bad mtu */
uint64_t sbe_term_frames_length(uint64_t len, uint32_t mtu);
size_t sbe_term_append_workspace_size(uint64_t n);
/* bytes of block one workgroup composes (a multiple of 32) */
uint32_t sbe_term_append_tile(void);
int sbe_term_append(const uint8_t* in, uint64_t in_bytes, const uint64_t* rec_off, uint64_t n, uint8_t* block,
                    uint64_t block_bytes, uint64_t start, uint64_t limit, uint32_t mtu, uint64_t max_message_length,
                    const sbe_term_header* hdr, const sbe_term_append_out* o, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ================== Record counts held in device memory (the *_counted calls) ================== */
/* The subscriber's egress step (polling_worker -> poll -> handle_incoming_message -> commit_message
 * -> send_commit_offset -> offer) without a host read between its stages: sbe_term_poll leaves its
 * message count in counts[4], the emit call its frame count in totals[0], and the calls below take
 * their record count from such a word.  The same rule in all four:
 *   n = min(*n_dev, n_capacity)
 * n_dev: a device const uint64_t*, 8-B aligned, read on `stream` by the launches that use it, so it
 * may be the output of an earlier launch on that stream.  n_capacity (host) lays out the grids, the
 * workspace and the block-sum tables: every array holds n_capacity records (rec_off n_capacity + 1
 * offsets), the workspace is the base call's *_workspace_size(n_capacity).
 * Results are those of the base call for n records.  No output element at a record index >= n is
 * written and no input element at a record index >= n is read: rec_off[n] is the last offset read,
 * rec_idx[j] is read for j < n only.  *n_dev == 0 is the base call's n == 0 (counts, totals,
 * out_off[0], last and count are written; the launches are those of n_capacity > 0).  n_capacity ==
 * 0: SBE_OK, the base call's n == 0 launch or memsets, n_dev is not read.  SBE_EINVAL (before
 * anything touches a device, and before SBE_ENOSPC): whatever the base call refuses with n =
 * n_capacity; a null or misaligned n_dev with n_capacity > 0; a misaligned rec_idx.  No call waits,
 * copies to the host or allocates.  A workgroup past the count exits behind one scalar load.
 *
 * sbe_decode_batch_counted: sbe_decode_batch_sized.  avg_record_bytes picks the window by that call's
 * thresholds on the average record size (0: the 16 KiB kernel); outputs are identical for any value.
 * out->seq is evaluated in the same launch.
 * sbe_classify_commits_counted: sbe_classify_commits; last and count are initialised by the call.
 * sbe_emit_commit_offsets_counted: sbe_emit_commit_offsets_ex (fb == NULL: sbe_emit_commit_offsets):
 * out_off[0..n], status[0..n), emit_idx[0..totals[0]) and totals.
 * sbe_term_append_counted: sbe_term_append over n records, where record j is in[rec_off[r] ..
 * rec_off[r + 1]) with r = rec_idx ? rec_idx[j] : j (rec_idx: device u64[n_capacity] or NULL; an r >=
 * n_capacity is a bad record).  rec_tail[j] and counts keep their meaning, indexed by j (with rec_idx
 * the payload bytes are added up with atomics).  With rec_off = res->out_off, rec_idx =
 * res->emit_idx, n_dev = res->totals and in_bytes = the emit call's out_capacity it appends exactly the
 * emitted frames: a frame reported SBE_CE_OVERFLOW ends past in_bytes, so it stops the append with
 * SBE_TERM_APPEND_BAD_RECORD, is not consumed, and nothing outside `in` is read. */
int sbe_decode_batch_counted(const uint8_t* in, const uint64_t* rec_off, const uint64_t* n_dev, uint64_t n_capacity,
                             uint64_t avg_record_bytes, uint32_t mode, const sbe_decoded* out, void* stream);
int sbe_classify_commits_counted(const uint8_t* in, const uint64_t* rec_off, const uint64_t* n_dev, uint64_t n_capacity,
                                 const sbe_decoded* dec, const uint8_t* topic_arena, const uint32_t* topic_off,
                                 uint32_t k, const sbe_commit_out* out, void* workspace, size_t workspace_bytes,
                                 void* stream);
int sbe_emit_commit_offsets_counted(const uint8_t* in, const uint64_t* rec_off, const uint64_t* n_dev,
                                    uint64_t n_capacity, const sbe_decoded* dec, const sbe_commit_out* plan,
                                    const uint32_t* topic_id, const uint8_t* ident_arena, const uint32_t* ident_off,
                                    uint32_t k, const uint8_t* mask, uint32_t flags, int session,
                                    int64_t leadership_term_id, int64_t cluster_session_id, uint8_t* out,
                                    uint64_t out_capacity, const sbe_commit_emit_out* res, void* workspace,
                                    size_t workspace_bytes, void* stream, const sbe_commit_fallback* fb);
int sbe_term_append_counted(const uint8_t* in, uint64_t in_bytes, const uint64_t* rec_off, const uint64_t* rec_idx,
                            const uint64_t* n_dev, uint64_t n_capacity, uint8_t* block, uint64_t block_bytes,
                            uint64_t start, uint64_t limit, uint32_t mtu, uint64_t max_message_length,
                            const sbe_term_header* hdr, const sbe_term_append_out* o, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ========================== Order JSON (publish_order payload) ========================== */
/* Replaces Order::to_json (src/order_types.cpp:122-181, jsoncpp StreamWriterBuilder with
 * indentation "" → compact, keys sorted) and the headers JSON publish_order builds beside it
 * (src/cluster_client.cpp:308-323), for a batch of Orders, so the strings feed
 * sbe_encode_topic_batch as payload / headers without a host round trip.
 * A batch of Orders (struct of arrays; order_types.hpp:16-66):
 *   arena, str_off ([n][8] or NULL = packed), str_len [n][8]: the string members
 *     0 client_order_uuid, 1 identifier, 2 base_token, 3 quote_token, 4 side, 5 id,
 *     6 message_id (OrderUtils::generate_message_id's value, made by the caller),
 *     7 status (selects messageType: "UPDATED" / "CANCELLED" → UPDATE_ORDER, else CREATE_ORDER);
 *   customer_id [n], timestamp [n] (ns; create_ts = timestamp / 1000000), quantity [n] (f64).
 * Number text follows glibc printf on the exact binary value: "%.17g" (jsoncpp valueToString,
 * ".0" appended when there is no '.' or 'e'; NaN → null, ±inf → ±1e+9999) and "%f"
 * (std::to_string); strings are escaped as jsoncpp 1.9.5 valueToQuotedStringN with emitUTF8
 * false (\" \\ \b \f \n \r \t, other controls and every non-ASCII code point as lower-case \uXXXX,
 * invalid UTF-8 as �); identifier is cut at its first NUL (.c_str(), order_types.cpp:138). */
#define SBE_ORDER_FIELDS 8u
#define SBE_JSON_ORDER_PAYLOAD 0u   /* Order::to_json() */
#define SBE_JSON_PUBLISH_HEADERS 1u /* {"messageId":…,"messageType":…,"orderId":…} */
#define SBE_JSON_OK 0u
#define SBE_JSON_OVERFLOW 6u        /* record ends past out_capacity (nothing written) */
typedef struct sbe_order_batch {
    const uint8_t* arena;
    const uint32_t* str_off;
    const uint32_t* str_len;
    const int64_t* customer_id;
    const int64_t* timestamp;
    const double* quantity;
} sbe_order_batch;

/* Bytes of device workspace sbe_order_to_json_batch needs for n records. */
size_t sbe_order_json_workspace_size(uint64_t n);

/* Write the JSON text of n Orders back to back: record i = out[out_off[i] .. out_off[i+1]).
 * out_off (n + 1 device u64) always holds the full sizes; a record past out_capacity is not
 * written and gets status SBE_JSON_OVERFLOW (status: n device u8 or NULL).  Alignment: out_off
 * 8 B, the Order arrays their natural alignment; out and arena need none.  On `stream`: a
 * sizing launch, a one-block scan of its per-block sums and the writing launch (packed arena:
 * first a per-block string-bytes launch and its scan). */
int sbe_order_to_json_batch(const sbe_order_batch* in, uint64_t n, uint32_t what, uint8_t* out,
                            uint64_t out_capacity, uint64_t* out_off, uint8_t* status, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ==================== publish_order: Orders straight to wire records ==================== */
/* ClusterClient::publish_order (src/cluster_client.cpp:300-333) and publish_order_to_topic
 * (:335-372) for a batch of Orders in one call.  Record i is what the reference offers for
 * order i: [the 32-B SessionMessageHeader {24,1,111,8, termId, sessionId, 0} when `session`]
 * the TopicMessage header {16,1,1,1}, the 16-B block (timestamp[i], 0 -> ts_default; sequence 0)
 * and the five u16-length-prefixed fields
 *   topic        one per call (device bytes),
 *   messageType  "UPDATE_ORDER" when status is "UPDATED" or "CANCELLED", else "CREATE_ORDER",
 *   uuid         the Order's message_id (field 6, made by the caller),
 *   payload      the Order::to_json text,
 *   headers      the {"messageId","messageType","orderId"} text,
 * byte for byte what sbe_order_to_json_batch (twice) followed by sbe_encode_topic_batch /
 * sbe_encode_session_batch produce, without the texts ever being written to memory on their own.
 * flags: 0 = the wire-correct 34 + Σlen bytes; SBE_ENC_REF_TRUNCATE8 = the 26 + Σlen bytes
 * create_topic_message returns (src/session_manager.cpp:1050-1115; the live path);
 * SBE_ENC_PUBLISH_TOPIC is refused (SBE_EINVAL): it is not publish_order's path.
 *
 * Per-record status, first match wins (a failing record emits 0 bytes, the batch goes on):
 *   SBE_PUB_INVALID_*   Order::validate() (src/order_types.cpp:66-120) ran first and its first
 *                       message is this one ("Order validation failed: " + errors[0]); only when
 *                       `checks` is given.  error_mask[i] (optional) has bit k set for every
 *                       message SBE_PUB_INVALID_ID + k validate() returns.
 *   SBE_ENC_E109_*      computeLength's order on the text lengths: topic, uuid (message_id),
 *                       payload text, headers text longer than 65534 bytes.
 *   SBE_ENC_OVERFLOW    the record ends past out_capacity (nothing is written past it).
 * Comparisons are the reference's: strings match exactly; `quantity <= 0.0` is false for NaN (a
 * NaN quantity passes) and true for -0.0. */
#define SBE_PUB_INVALID_ID 16u               /* "Order ID is required" */
#define SBE_PUB_INVALID_BASE_TOKEN 17u       /* "Base token is required" */
#define SBE_PUB_INVALID_QUOTE_TOKEN 18u      /* "Quote token is required" */
#define SBE_PUB_INVALID_SIDE 19u             /* "Side must be 'BUY' or 'SELL'" */
#define SBE_PUB_INVALID_QUANTITY 20u         /* "Quantity must be positive" */
#define SBE_PUB_INVALID_ORDER_TYPE 21u       /* "Invalid order type: " + order_type */
#define SBE_PUB_INVALID_LIMIT_PRICE 22u      /* "Limit price must be positive for LIMIT orders" */
#define SBE_PUB_INVALID_STOP_PRICE 23u       /* "Stop price must be positive for STOP orders" */
#define SBE_PUB_INVALID_STOP_LIMIT_STOP 24u  /* "Stop price must be positive for STOP_LIMIT orders" */
#define SBE_PUB_INVALID_STOP_LIMIT_LIMIT 25u /* "Limit price must be positive for STOP_LIMIT orders" */
#define SBE_PUB_INVALID_TIME_IN_FORCE 26u    /* "Invalid time in force: " + time_in_force */
#define SBE_PUB_INVALID_GTD_EXPIRY 27u       /* "Expiry timestamp required for GTD orders" */
#define SBE_PUB_INVALID_COUNT 12u

/* The Order members only validate() reads (order_types.hpp:28-49), struct of arrays:
 *   arena, str_off ([n][2] or NULL = packed), str_len [n][2]: order_type, time_in_force;
 *   limit_price [n], stop_price [n] (f64);
 *   present [n] u8: bit 0 = stop_price has a value, bit 1 = expiry_timestamp has a value. */
#define SBE_PUB_HAS_STOP_PRICE 0x1u
#define SBE_PUB_HAS_EXPIRY 0x2u
typedef struct sbe_order_checks {
    const uint8_t* arena;
    const uint32_t* str_off;
    const uint32_t* str_len;
    const double* limit_price;
    const double* stop_price;
    const uint8_t* present;
} sbe_order_checks;

/* Bytes of device workspace sbe_publish_orders_batch needs for n Orders (at most 64 n + 65536:
 * it holds sizes and offsets only, no text). */
size_t sbe_publish_orders_workspace_size(uint64_t n);

/* Upper bound of the record stream of n Orders whose Order strings total `string_bytes` (every
 * string byte escapes to at most 6 text bytes and is printed at most three times).  A tighter
 * size: call once with out = NULL, out_capacity = 0 and read out_off[n], which always holds the
 * full layout. */
uint64_t sbe_publish_orders_output_bound(uint64_t n, uint64_t string_bytes, uint32_t topic_len, int session);

/* orders: as for sbe_order_to_json_batch.  checks: NULL skips validation (the caller has
 * validated).  topic: topic_len device bytes (NULL only when topic_len is 0).  timestamp: [n]
 * device u64 or NULL (every record takes ts_default).  session: 0 bare TopicMessage, 1 framed.
 * out (16-B aligned; NULL with out_capacity 0 sizes only), out_off [n + 1] (8-B aligned, always
 * the full layout), status [n] u8 or NULL, error_mask [n] u16 (2-B aligned) or NULL, workspace
 * (16-B aligned) as for the sibling encoders.  Every argument is checked before anything is
 * launched; n == 0 is SBE_OK with out_off[0] = 0.  On `stream`: per-block totals and their scans
 * (packed arenas), the sizing launch, one scan, the writing launch. */
int sbe_publish_orders_batch(const sbe_order_batch* orders, const sbe_order_checks* checks, uint64_t n,
                             const uint8_t* topic, uint32_t topic_len, const uint64_t* timestamp,
                             uint64_t ts_default, uint32_t flags, int session, int64_t leadership_term_id,
                             int64_t cluster_session_id, uint8_t* out, uint64_t out_capacity, uint64_t* out_off,
                             uint8_t* status, uint16_t* error_mask, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ======================= multi-GPU gather of encoded shards (RCCL) ======================= */
/* A batch sharded over the GPUs of one node (records [lo_r, hi_r) on rank r, contiguous, in rank
 * order) is encoded per rank with no collective; sbe_gather_encoded then assembles on one rank the
 * stream and offsets a single-GPU encode of the whole batch produces, over RCCL (xGMI inside a
 * node).  The reference has no counterpart: its only transport is Aeron
 * (src/session_manager.cpp:1180); the gathered stream is what one ingress publisher offers
 * record by record (ClusterClient::offer_ingress, include/aeron_cluster/cluster_client.hpp:409).
 * One process per GPU; a communicator serves one stream at a time. */
#define SBE_ECOMM (-5)       /* an RCCL call failed (sbe_last_error names it) */
#define SBE_COMM_ID_BYTES 128u
typedef struct sbe_comm sbe_comm;

/* A fresh communicator id (ncclGetUniqueId), made on one rank and passed to every rank out of band. */
int sbe_comm_unique_id(uint8_t id[SBE_COMM_ID_BYTES]);
/* Collective over the `world` processes: create this rank's communicator on the current HIP device. */
int sbe_comm_init(sbe_comm** comm, int world, int rank, const uint8_t id[SBE_COMM_ID_BYTES]);
int sbe_comm_destroy(sbe_comm* comm);

/* Collective over the communicator.  Every rank passes its shard: out (its encoded stream, 16-B
 * aligned) with out_off [n+1] (device u64, out_off[0] == 0) as sbe_encode_*_batch wrote them.
 * The root receives the shards back to back in rank order into dst (dst_capacity bytes) and the
 * rebased offsets into dst_off (dst_off_capacity device u64 entries; N + 1 are written, N = Σ n_r:
 * record j of rank r at Σ_{q<r} bytes_q + out_off_r[j]); other ranks pass dst = dst_off = NULL and
 * capacities 0.  totals (host u64[2], or NULL) = {Σ bytes, N} on every rank.  On `stream`: an
 * all-gather of the ranks' {bytes, n, root capacities}, one 32-B-per-rank device→host copy and a
 * synchronisation of `stream` (the root sizes its receives from it), the plan of sbe_gather_plan,
 * then one group of ncclSend / ncclRecv at the prefix offsets (RCCL has no gatherv) and the root's
 * offset rebase; returns once those are enqueued.  SBE_ENOSPC on every rank (nothing sent) when the
 * root's dst or dst_off is too small.  RCCL is loaded on the first sbe_comm_* call (the RCCL the
 * process already holds, else librccl.so.1); nothing else in this library needs it. */
int sbe_gather_encoded(sbe_comm* comm, int root, const uint8_t* out, const uint64_t* out_off, uint64_t n,
                       uint8_t* dst, uint64_t dst_capacity, uint64_t* dst_off, uint64_t dst_off_capacity,
                       uint64_t* totals, void* stream);

/* The same gather for a caller that already knows every rank's shard size (fixed-size records:
 * bytes = records x record size; or the host size plan the C++ mirror keeps for every encode):
 * sizes (host u64 [world][2]) = {bytes, records} of each rank's shard, identical on every rank.
 * No size all-gather and no host synchronisation: it enqueues the grouped ncclSend / ncclRecv and
 * the root's rebase on `stream` and returns, so a rank can go on to encode its next shard while
 * this one travels.  dst_capacity / dst_off_capacity are the ROOT's capacities, passed on every
 * rank (non-roots pass dst = dst_off = NULL), so every rank reaches the same SBE_ENOSPC verdict
 * before anything is sent; dst_off_capacity 0 is SBE_EINVAL (N + 1 >= 1 offsets are always
 * written), and a rank that passes other capacities than the root's can leave the root blocked in
 * its receives, so the Python binding refuses zero capacities on every rank.  The sizes are trusted as a planned encode's tile sums are: they must
 * equal out_off[n] and n of the shard each rank encoded (a wrong plan moves the wrong bytes; it
 * never writes past the root's capacities). */
int sbe_gather_encoded_sized(sbe_comm* comm, int root, const uint64_t* sizes, const uint8_t* out,
                             const uint64_t* out_off, uint8_t* dst, uint64_t dst_capacity, uint64_t* dst_off,
                             uint64_t dst_off_capacity, uint64_t* totals, void* stream);

/* The gather's plan (host only, no device): from every rank's {bytes, records, dst_capacity,
 * dst_off_capacity} (ranks: host u64 [world][4], the capacities read from the root's entry) the
 * byte and record base of each rank's shard on the root (byte_base / rec_base: host u64
 * [world + 1], exclusive prefix sums; the last entry is the total) and totals {Σ bytes, Σ records}
 * (or NULL).  SBE_ENOSPC when the root's dst holds fewer than Σ bytes or its dst_off fewer than
 * Σ records + 1 entries; SBE_EINVAL on a bad world / root. */
int sbe_gather_plan(const uint64_t* ranks, int world, int root, uint64_t* byte_base, uint64_t* rec_base,
                    uint64_t* totals);

/* ============================ small-batch serve kernel ============================ */
/* A one-record call through the batch entry points pays a kernel launch and a completion wait
 * (≈12 us round trip on MI355X, profiles/r04_launch_probe.log) on top of its few microseconds of
 * work: the reference's per-message calls (SBEEncoder::encode_topic_message,
 * src/sbe_encoder.cpp:131-181; SBEDecoder/parse_message, src/sbe_encoder.cpp:183-318 and
 * 915-1029; ClusterClient::publish_topic, src/cluster_client.cpp:1850-1857) cost well under that
 * on a CPU.  A server is one resident workgroup on its own HIP stream that polls a page-locked
 * request slot and runs each small batch as it arrives (no launch per request, ≈3 us round
 * trip), then exits after `idle_us` without a request; the next request relaunches it.
 * Every sbe_serve_* call is synchronous: it returns when the outputs are written (or with the
 * error the batch entry point would return, checked on the host before posting).  Outputs are
 * byte-identical to the batch entry points'.  Pointers are device-visible addresses (device
 * memory, or page-locked host memory's device pointer); encodes take packed input only
 * (str_off == NULL); n <= SBE_SERVE_MAX_RECORDS (one workgroup walks the batch tile by tile, so
 * large batches belong on the batch entry points).  A server is used by one host thread at a time. */
#define SBE_SERVE_MAX_RECORDS 4096u
typedef struct sbe_server sbe_server;
/* idle_us: how long the resident kernel waits for a request before it exits (0: 1000).  Keep it
 * short: see sbe_server_quiesce on what a resident server holds up. */
int sbe_server_create(sbe_server** srv, uint32_t idle_us);
/* A server of `workgroups` resident workgroups (1..SBE_SERVE_MAX_WORKGROUPS): workgroup 0 polls the
 * slot and republishes a request of several tiles to the others through device memory; a decode
 * of T tiles (64 records each) then runs on min(T, workgroups) of them, as does a planned encode
 * (below).  One-tile requests run on workgroup 0 alone, as with sbe_server_create. */
#define SBE_SERVE_MAX_WORKGROUPS 64u
int sbe_server_create_wide(sbe_server** srv, uint32_t idle_us, uint32_t workgroups);
/* Stops the kernel (a shutdown request, then the stream is synchronised) and frees the server.
 * A request that times out (10 s) or finds the server's stream failed returns SBE_EHIP and leaves
 * the server failed: every later request returns SBE_EHIP at once, and destroy only waits for the
 * kernel to leave (it exits idle_us after its last request) before freeing.  That wait is bounded
 * (idle_us + 10 s): a kernel still running then is left with its buffers (never freed under it)
 * and destroy returns SBE_EHIP. */
int sbe_server_destroy(sbe_server* srv);
int sbe_serve_encode_topic(sbe_server* srv, const sbe_tm_batch* in, uint64_t n, uint64_t ts_default, uint32_t flags,
                           uint8_t* out, uint64_t out_capacity, uint64_t* out_off, uint8_t* status);
int sbe_serve_encode_session(sbe_server* srv, const sbe_tm_batch* in, uint64_t n, uint64_t ts_default,
                             uint32_t flags, int64_t leadership_term_id, int64_t cluster_session_id, uint8_t* out,
                             uint64_t out_capacity, uint64_t* out_off, uint8_t* status);
int sbe_serve_encode_lite(sbe_server* srv, const sbe_lite_batch* in, uint64_t n, uint32_t template_id, uint8_t* out,
                          uint64_t out_capacity, uint64_t* out_off, uint8_t* status);
/* sbe_decode_batch's modes and outputs (seq evaluated in the same request when non-NULL). */
int sbe_serve_decode(sbe_server* srv, const uint8_t* in, const uint64_t* rec_off, uint64_t n, uint32_t mode,
                     const sbe_decoded* out);
/* The same with the inputs in host memory (any memory the calling thread reads; packed strings,
 * no alignment needed): they are copied into the server's request slot, and the kernel moves them
 * to device scratch in the round trip that fetches the request, so its dependent reads (offsets,
 * then records; lengths, then strings) hit the L2 instead of crossing PCIe twice.  At most
 * SBE_SERVE_INLINE_BYTES of inputs per request, laid out 16-B aligned: decode
 * 8 (n + 1) + (rec_off[n] - rec_off[0]); encode Σlen + 4 nf n + 8 n (+ 4 n Lite topicIds).
 * SBE_EINVAL when they do not fit.  Outputs are device-visible pointers, as above. */
#define SBE_SERVE_INLINE_BYTES 16384u
int sbe_serve_encode_topic_host(sbe_server* srv, const sbe_tm_batch* in, uint64_t n, uint64_t ts_default,
                                uint32_t flags, uint8_t* out, uint64_t out_capacity, uint64_t* out_off,
                                uint8_t* status);
int sbe_serve_encode_session_host(sbe_server* srv, const sbe_tm_batch* in, uint64_t n, uint64_t ts_default,
                                  uint32_t flags, int64_t leadership_term_id, int64_t cluster_session_id,
                                  uint8_t* out, uint64_t out_capacity, uint64_t* out_off, uint8_t* status);
int sbe_serve_encode_lite_host(sbe_server* srv, const sbe_lite_batch* in, uint64_t n, uint32_t template_id,
                               uint8_t* out, uint64_t out_capacity, uint64_t* out_off, uint8_t* status);
int sbe_serve_decode_host(sbe_server* srv, const uint8_t* in, const uint64_t* rec_off, uint64_t n, uint32_t mode,
                          const sbe_decoded* out);
/* Planned encodes: device-visible inputs (packed) plus the tile sums sbe_encode_*_batch's first
 * launch would compute, supplied by a caller that knows every record's sizes (the C++ mirror
 * does): tile_sums [T][2] = output / input bytes before tile t inside its superblock, sb_sums
 * [S][2] = output / input bytes of superblock s, with T = ceil(n / R) tiles of R =
 * sbe_encode_tile_records(layout) records and superblocks of 128 R records; a record's output
 * bytes are 0 for an E109 record, its input bytes the sum of its string lengths.  The tile loop
 * of the batch kernel then runs on min(T, workgroups) workgroups.  Outputs are byte-identical.
 * The sums are trusted as the lengths are: output stores stay inside out_capacity whatever they
 * say, but input reads follow them, so sums that do not match the lengths read past the arena
 * (undefined, as lengths that overrun the arena are for every encode entry point). */
#define SBE_LAYOUT_TOPIC 0u
#define SBE_LAYOUT_SESSION 1u
#define SBE_LAYOUT_LITE 2u
uint32_t sbe_encode_tile_records(uint32_t layout);
int sbe_serve_encode_topic_planned(sbe_server* srv, const sbe_tm_batch* in, uint64_t n, uint64_t ts_default,
                                   uint32_t flags, uint8_t* out, uint64_t out_capacity, uint64_t* out_off,
                                   uint8_t* status, const uint64_t* tile_sums, const uint64_t* sb_sums);
int sbe_serve_encode_session_planned(sbe_server* srv, const sbe_tm_batch* in, uint64_t n, uint64_t ts_default,
                                     uint32_t flags, int64_t leadership_term_id, int64_t cluster_session_id,
                                     uint8_t* out, uint64_t out_capacity, uint64_t* out_off, uint8_t* status,
                                     const uint64_t* tile_sums, const uint64_t* sb_sums);
int sbe_serve_encode_lite_planned(sbe_server* srv, const sbe_lite_batch* in, uint64_t n, uint32_t template_id,
                                  uint8_t* out, uint64_t out_capacity, uint64_t* out_off, uint8_t* status,
                                  const uint64_t* tile_sums, const uint64_t* sb_sums);
/* Makes a resident server exit now (a shutdown request, then its stream is synchronised) and
 * keeps it usable: the next request relaunches it.  SBE_OK at once when it is not running.
 *
 * WHY THIS MATTERS.  While its kernel is resident (from a request until idle_us after the last
 * one), a server occupies a HIP hardware queue, and HIP maps streams onto GPU_MAX_HW_QUEUES
 * queues (4 by default) shared by every stream of the process.  Work on a stream that shares the
 * server's queue, and any device-wide synchronisation (hipDeviceSynchronize,
 * torch.cuda.synchronize()), waits until the server exits: up to idle_us after its last request,
 * and for as long as its owner keeps it busy.  Quiesce the thread's server before such a
 * synchronisation or before enqueueing large work; keep idle_us short (the C++ mirror's default is
 * 1 ms, and the mirror quiesces its own server before every batch it launches). */
int sbe_server_quiesce(sbe_server* srv);
/* Requests this server ran and kernel launches it took (a launch per idle exit). */
int sbe_server_stats(const sbe_server* srv, uint64_t* requests, uint64_t* launches);

/* ================================== profiling ================================== */
/* Optional (off by default; thread-local): sbe_profile_enable(every) with every >= 1 makes every
 * `every`-th sbe_encode_topic_batch / sbe_decode_batch call of this thread carry a pair of HIP
 * events on its main kernel's dispatch (kernel 0 = the encode pack kernel, 1 = the decode
 * kernel; hipExtLaunchKernel timestamps), kept in a ring of the last 256 per kernel; 0 turns it
 * off.  Each call resets the rings and launch counters (the first enabling call creates the events,
 * so none is created inside a timed region; SBE_EHIP when they cannot be created, e.g. no device).  sbe_profile_read copies the elapsed
 * milliseconds of up to `max` most recent sampled launches (oldest first) into ms[], clears the
 * ring and returns the count; the caller synchronises the streams first.  Used by bench.py to
 * time the dominant kernel inside its timed region (a timed dispatch costs the GPU several us,
 * hence the sampling). */
int sbe_profile_enable(int every);
int sbe_profile_read(int kernel, float* ms, int max);

/* ===================================== misc ===================================== */
int sbe_abi_version(void);
/* 1 if a gfx950 device is visible to HIP, 0 if not, <0 on HIP error. */
int sbe_device_ready(void);
/* Name of the last HIP error seen by this library (thread-local), "" if none. */
const char* sbe_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SBECODEC_H */
