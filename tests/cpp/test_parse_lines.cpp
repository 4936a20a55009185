// Prints one canonical line (oracle/parse_line.hpp) per record of a file from the host mirror's
// functions, for tests that compare the lines with the same header's lines from the reference's
// own compiled source (oracle/ref_sources.cpp: refsrc_describe).
//
//   test_parse_lines FILE bytes    the helpers that read the record's bytes alone (no device)
//   test_parse_lines FILE single   MessageParser::parse_message per record, the bytes part, and
//                                  is_acknowledgment_for (device)
//   test_parse_lines FILE batch    MessageParser::parse_batch over the whole file (device)
//
// FILE: u64 n, u64 bytes, u64 rec_off[n + 1], the records back to back.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "aeron_cluster_amd.hpp"
#include "../../oracle/parse_line.hpp"

using namespace aeron_cluster;

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s FILE bytes|single|batch\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    uint64_t head[2];
    if (!f || std::fread(head, 8, 2, f) != 2) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const uint64_t n = head[0], bytes = head[1];
    std::vector<uint64_t> off(n + 1);
    std::vector<uint8_t> data(bytes + 16, 0);
    if (std::fread(off.data(), 8, n + 1, f) != n + 1 || std::fread(data.data(), 1, bytes, f) != bytes || off[n] != bytes) {
        std::fprintf(stderr, "short or inconsistent file %s\n", argv[1]);
        return 2;
    }
    std::fclose(f);
    const std::string mode = argv[2];
    std::string out;
    if (mode == "batch") {
        const std::vector<ParseResult> res = MessageParser::parse_batch(data.data(), off.data(), n);
        if (res.size() != n) return 3;
        for (const ParseResult& r : res) out += parse_line::of_result(r) + "\n";
    } else if (mode == "single" || mode == "bytes") {
        for (uint64_t i = 0; i < n; ++i) {
            const uint8_t* rec = data.data() + off[i];
            const size_t len = off[i + 1] - off[i];
            if (mode == "single") {
                const ParseResult r = MessageParser::parse_message(rec, len);
                out += parse_line::of_result(r) + " " + parse_line::of_bytes(rec, len) + " " +
                       parse_line::of_ack_for(rec, len, r.message_id) + "\n";
            } else {
                out += parse_line::of_bytes(rec, len) + "\n";
            }
        }
    } else {
        return 2;
    }
    std::fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
