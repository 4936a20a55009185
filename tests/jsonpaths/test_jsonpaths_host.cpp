// The host mirror's JSON extraction over files tests/test_gpu_jsonpaths_host.py writes and checks
// against the restatement (paths_ref.cpp).  Modes:
//   orders  <in> <out>  records → MessageParser::decode_batch → extract_order_ids: two strings per
//                       record; then ParsedBatch::extract of the headers' "messageType" (view 4, every
//                       third record deselected): kind and as_string per record.  The one-record
//                       form extract_order_ids(ParseResult) must agree on the first 64 records.
//   fields  <in> <out>  a path table and bare documents → extract_json_documents: doc, root_kind and
//                       per path kind, is_string, token, as_string and as_uint64 (or that they throw)
//   offsets <in> <out>  documents → CommitManager::parse_commit_offsets_batch with errors: per
//                       document 0 + the five members, 1 a parse failure, 2 another exception;
//                       parse_commit_offset must agree on the first 40
// Strings are u32-length-prefixed, integers little-endian.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "aeron_cluster_amd.hpp"

using namespace aeron_cluster;

static std::uint32_t get_u32(FILE* f) {
    std::uint32_t v = 0;
    if (std::fread(&v, 4, 1, f) != 1) throw std::runtime_error("short file");
    return v;
}
static std::string get_str(FILE* f) {
    std::string s(get_u32(f), '\0');
    if (!s.empty() && std::fread(&s[0], 1, s.size(), f) != s.size()) throw std::runtime_error("short file");
    return s;
}
static void put_u8(FILE* f, std::uint8_t v) { std::fputc(v, f); }
static void put_u64(FILE* f, std::uint64_t v) { std::fwrite(&v, 8, 1, f); }
static void put_str(FILE* f, std::string_view s) {
    const std::uint32_t n = (std::uint32_t)s.size();
    std::fwrite(&n, 4, 1, f);
    std::fwrite(s.data(), 1, s.size(), f);
}
static std::vector<std::string> get_strs(FILE* f) {
    std::vector<std::string> v(get_u32(f));
    for (auto& s : v) s = get_str(f);
    return v;
}

static int orders(FILE* in, FILE* out) {
    const std::vector<std::string> recs = get_strs(in);
    std::string data;
    std::vector<std::uint64_t> off{0};
    for (const auto& r : recs) {
        data += r;
        off.push_back(data.size());
    }
    data.resize(data.size() + 16);
    const auto* p = reinterpret_cast<const std::uint8_t*>(data.data());
    const ParsedBatch batch = MessageParser::decode_batch(p, off.data(), recs.size());
    const std::vector<OrderIds> ids = extract_order_ids(batch);
    for (const OrderIds& o : ids) {
        put_str(out, o.client_order_id);
        put_str(out, o.order_id);
    }
    for (size_t i = 0; i < recs.size() && i < 64; ++i) {
        const OrderIds one = extract_order_ids(batch.result(i));
        if (one.client_order_id != ids[i].client_order_id || one.order_id != ids[i].order_id) {
            std::fprintf(stderr, "record %zu: the one-record form differs from the batch\n", i);
            return 1;
        }
    }
    std::vector<std::uint8_t> select(recs.size());
    for (size_t i = 0; i < recs.size(); ++i) select[i] = i % 3 != 2;
    const JsonFields h = batch.extract({JsonPath("messageType")}, 4, select.data());
    for (size_t i = 0; i < recs.size(); ++i) {
        put_u8(out, h.doc(i));
        put_u8(out, h.kind(i, 0));
        put_str(out, h.is_string(i, 0) ? h.as_string(i, 0) : std::string());
    }
    if (extract_order_ids(MessageParser::decode_batch(p, off.data(), 0)).size() != 0) return 1;
    return 0;
}

static int fields(FILE* in, FILE* out) {
    std::vector<JsonPath> paths;
    for (std::uint32_t P = get_u32(in); P; --P) paths.emplace_back(get_strs(in));
    const std::vector<std::string> docs = get_strs(in);
    const JsonFields f = extract_json_documents(docs, paths);
    if (f.size() != docs.size() || f.paths() != paths.size()) return 1;
    for (size_t i = 0; i < docs.size(); ++i) {
        put_u8(out, f.doc(i));
        put_u8(out, f.root_kind(i));
        for (size_t p = 0; p < paths.size(); ++p) {
            put_u8(out, f.kind(i, p));
            put_u8(out, f.is_string(i, p));
            put_str(out, f.token(i, p));
            try {
                const std::string s = f.as_string(i, p);
                put_u8(out, 0);
                put_str(out, s);
            } catch (const std::runtime_error&) {
                put_u8(out, 1);
                put_str(out, "");
            }
            try {
                const std::uint64_t v = f.as_uint64(i, p);
                put_u8(out, 0);
                put_u64(out, v);
            } catch (const std::runtime_error&) {
                put_u8(out, 1);
                put_u64(out, 0);
            }
        }
    }
    for (const char* bad : {"a..b", "", "a.b.c.d.e"}) {  // an empty name, five names
        try {
            extract_json_documents(docs, {JsonPath(bad)});
            std::fprintf(stderr, "path '%s' was accepted\n", bad);
            return 1;
        } catch (const std::invalid_argument&) {
        }
    }
    return 0;
}

static int offsets(FILE* in, FILE* out) {
    const std::vector<std::string> docs = get_strs(in);
    std::vector<std::string> errors;
    const std::vector<CommitOffset> got = CommitManager::parse_commit_offsets_batch(docs, &errors);
    const std::string prefix = "Failed to parse commit offset JSON: ";
    for (size_t i = 0; i < docs.size(); ++i) {
        const int code = errors[i].empty() ? 0 : errors[i].compare(0, prefix.size(), prefix) == 0 ? 1 : 2;
        put_u8(out, (std::uint8_t)code);
        put_str(out, got[i].topic);
        put_str(out, got[i].message_identifier);
        put_str(out, got[i].message_id);
        put_u64(out, got[i].timestamp_nanos);
        put_u64(out, got[i].sequence_number);
        if (i >= 40) continue;
        try {
            const CommitOffset o = CommitManager::parse_commit_offset(docs[i]);
            if (code != 0 || o.topic != got[i].topic || o.message_identifier != got[i].message_identifier ||
                o.message_id != got[i].message_id || o.timestamp_nanos != got[i].timestamp_nanos ||
                o.sequence_number != got[i].sequence_number) {
                std::fprintf(stderr, "document %zu: parse_commit_offset differs from the batch\n", i);
                return 1;
            }
        } catch (const std::runtime_error& e) {
            if (errors[i] != e.what()) {
                std::fprintf(stderr, "document %zu: '%s' against the batch's '%s'\n", i, e.what(), errors[i].c_str());
                return 1;
            }
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (argc != 4) return 2;
        const std::string mode = argv[1];
        FILE* in = std::fopen(argv[2], "rb");
        FILE* out = std::fopen(argv[3], "wb");
        if (!in || !out) return 2;
        const int rc = mode == "orders" ? orders(in, out) : mode == "fields" ? fields(in, out) : mode == "offsets" ? offsets(in, out) : 2;
        std::fclose(in);
        std::fclose(out);
        quiesce();
        if (rc) return rc;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::puts("jsonpaths host: ok");
    return 0;
}
