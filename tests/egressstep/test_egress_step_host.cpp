// EgressCommitter::poll_commit_append (one enqueue: sbe_term_poll and the four *_counted calls)
// beside the composition that defines its result: FragmentReassembler::poll_term_block, then
// MessageParser::decode_batch, AutoCommitter::commit_and_send_batch (json_fallback, session frames)
// into a list of frames, then TermAppender::append of those frames but for the records the step
// reports as left to the host.  The blocks of the case file (tests/termscan_lib.py, write_cases)
// are polled one after another by one object of each kind, so that a message that spans two blocks
// goes through the carry of both, and every step appends behind the one before it in one ingress
// block.  After every block the two must agree on *next, the pending accumulator, the message
// count, the frames' records, the append's result and the ingress bytes.  Prints one line per case
// and "egress step host: ok" with exit status 0.  A second argument is the ingress block's bytes
// (default 1 MiB, which never fills): with a small one the append trips, the step's padding-frame
// header and appended < frames are compared too, and both sides go on at offset 64 as in a new term.
//
// With --throws (no device needed): the argument checks that throw before anything is enqueued.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "aeron_cluster_amd.hpp"
#include "sbecodec.h"

using namespace aeron_cluster;

template <class T>
static bool rd(FILE* f, std::vector<T>& v, std::uint64_t count) {
    v.resize(count);
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

template <class E, class F>
static bool throws(F&& fn) {
    try {
        fn();
    } catch (const E&) {
        return true;
    } catch (...) {
    }
    return false;
}

static int check_throws() {
    std::vector<std::uint8_t> blk(256), ing(4096);
    EgressCommitter e("client-1", "orders");
    auto step = [&](std::size_t len, std::size_t start, std::size_t ilen, std::size_t istart, const EgressStepOptions& o) {
        return [&, len, start, ilen, istart] { e.poll_commit_append(blk.data(), len, start, ing.data(), ilen, istart, o); };
    };
    EgressStepOptions o, mtu = o, maxlen = o;
    mtu.append.mtu = 1400;
    maxlen.append.max_message_length = (1ull << 30) + 1;
    int bad = 0;
    bad += !throws<std::invalid_argument>(step(250, 0, 4096, 0, o));    // poll_term_block's
    bad += !throws<std::invalid_argument>(step(256, 8, 4096, 0, o));
    bad += !throws<std::invalid_argument>(step(256, 288, 4096, 0, o));
    bad += !throws<std::invalid_argument>(step(256, 0, 4090, 0, o));    // TermAppendOptions::check's
    bad += !throws<std::invalid_argument>(step(256, 0, 4096, 8, o));
    bad += !throws<std::invalid_argument>(step(256, 0, 4096, 4128, o));
    bad += !throws<std::invalid_argument>(step(256, 0, 4096, 0, mtu));
    bad += !throws<std::invalid_argument>(step(256, 0, 4096, 0, maxlen));
    EgressCommitter big(std::string(SBE_COMMIT_TABLE_BYTES + 1, 'c'));  // AutoCommitter::run's, with json_fallback
    bad += !throws<std::length_error>([&] { big.poll_commit_append(blk.data(), 256, 0, ing.data(), 4096, 0); });
    EgressCommitter idents("c");
    idents.set_message_identifier("alpha", std::string(3000, 'a'));
    idents.set_message_identifier("beta", std::string(3000, 'b'));
    bad += !throws<std::length_error>([&] { idents.poll_commit_append(blk.data(), 256, 0, ing.data(), 4096, 0); });
    bad += !throws<std::length_error>([] { EgressCommitter x("c", std::string(SBE_COMMIT_TABLE_BYTES + 1, 't')); });
    bad += !throws<std::length_error>([] {
        EgressCommitter x("c");
        for (int j = 0; j < 64; ++j) x.set_message_identifier("topic-" + std::to_string(j), "i");
    });
    if (bad) {
        std::printf("egress step throws: %d checks failed\n", bad);
        return 1;
    }
    std::printf("egress step throws: ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 64;
    if (std::strcmp(argv[1], "--throws") == 0) return check_throws();
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::uint64_t count = 0;
    if (std::fread(&count, 8, 1, f) != 1) return 3;
    const std::size_t ingress_len = argc > 2 ? (std::size_t)std::strtoull(argv[2], nullptr, 10) : (std::size_t)1 << 20;
    std::vector<std::uint8_t> got_blk(ingress_len, 0xA5), exp_blk(ingress_len, 0xA5);
    EgressCommitter step("client-7", "default");
    AutoCommitter ac("client-7", "default");
    for (auto* p : {"alpha", "beta", "orders", "order_request_topic"}) {
        step.set_message_identifier(p, std::string("sub-") + p);
        ac.set_message_identifier(p, std::string("sub-") + p);
    }
    FragmentReassembler poll;
    TermAppender appender;
    CommitManager commits;
    std::uint64_t clock_at = 0;
    EgressStepOptions o;
    o.leadership_term_id = 3;
    o.cluster_session_id = 4;
    o.append.header = TermHeader{5, 6, 7, 4096, 1};
    std::size_t tail_got = 64, tail_exp = 64;
    int bad = 0;
    for (std::uint64_t k = 0; k < count; ++k) {
        std::uint64_t h[6];
        std::vector<std::uint8_t> block, flags;
        std::vector<std::uint64_t> frag_off;
        std::vector<std::uint32_t> frag_src;
        if (std::fread(h, 8, 6, f) != 6) return 3;
        if (!rd(f, block, h[0]) || !rd(f, frag_off, h[3] + 1) || !rd(f, frag_src, h[3]) || !rd(f, flags, h[3])) return 4;
        const std::size_t limit = h[2] >= (1ull << 62) ? ~(std::size_t)0 : (std::size_t)h[2];
        // the composition
        std::size_t next_exp = 0;
        const EncodedBatch msgs = poll.poll_term_block(block.data(), block.size(), h[1], limit, &next_exp);
        const std::size_t m = msgs.offsets.size() ? msgs.offsets.size() - 1 : 0;
        const ParsedBatch parsed = MessageParser::decode_batch(msgs.bytes.data(), msgs.offsets.data(), m);
        std::vector<std::vector<std::uint8_t>> offered;
        CommitSendOptions so;
        so.leadership_term_id = 3;
        so.cluster_session_id = 4;
        so.json_fallback = true;
        const std::uint64_t c0 = clock_at;
        so.clock = [&] { return 1000 + clock_at++; };
        const CommitSendResult sent = ac.commit_and_send_batch(
            parsed, commits, [&](const std::uint8_t* p, std::size_t n) { offered.emplace_back(p, p + n); return true; }, so);
        // the step, on the same clock readings
        clock_at = c0;
        o.limit = limit;
        o.clock = so.clock;
        EncodedBatch step_msgs;
        const EgressStepResult r = step.poll_commit_append(block.data(), block.size(), h[1], got_blk.data(), ingress_len, tail_got, o, &step_msgs);
        // the records behind the offered frames: the device's and the host-resolved ones that were sent
        std::vector<std::size_t> skip(sent.too_long);
        skip.insert(skip.end(), sent.fallback_e100.begin(), sent.fallback_e100.end());
        std::vector<std::pair<std::size_t, bool>> order;  // record, from the device
        for (std::size_t i : r.frame_record) order.emplace_back(i, true);
        for (std::size_t i : r.host)
            if (std::find(skip.begin(), skip.end(), i) == skip.end()) order.emplace_back(i, false);
        std::sort(order.begin(), order.end());
        bool same = order.size() == offered.size() && r.next == next_exp && r.messages == m &&
                    step.pending_bytes() == poll.pending_bytes() && r.frames == r.frame_record.size() &&
                    step_msgs.bytes.size() == msgs.bytes.size() && step_msgs.offsets.size() == msgs.offsets.size() &&
                    (msgs.bytes.size() == 0 || std::memcmp(step_msgs.bytes.data(), msgs.bytes.data(), msgs.bytes.size()) == 0);
        std::vector<std::uint8_t> dense;
        std::vector<std::uint64_t> off{0};
        if (same)
            for (std::size_t j = 0; j < order.size(); ++j)
                if (order[j].second) {
                    dense.insert(dense.end(), offered[j].begin(), offered[j].end());
                    off.push_back(dense.size());
                }
        const TermAppendResult a = appender.append(dense.data(), dense.size(), off.data(), off.size() - 1, exp_blk.data(), ingress_len,
                                                   tail_exp, o.append);
        same = same && a.appended == r.appended.appended && a.next == r.appended.next && a.stop == r.appended.stop &&
               a.rec_tail == r.appended.rec_tail && (a.stop == SBE_TERM_APPEND_END ? a.appended == r.frames : a.appended < r.frames) &&
               got_blk == exp_blk;
        std::printf("case %llu: messages %zu frames %llu host %zu pending %zu next %zu tail %llu stop %u appended %zu%s\n",
                    (unsigned long long)k, m, (unsigned long long)r.frames, r.host.size(), step.pending_bytes(), r.next,
                    (unsigned long long)r.appended.next, r.appended.stop, r.appended.appended,
                    same ? "" : "  DIFFERS from the composed calls");
        if (!same) ++bad;
        const bool tripped = r.appended.stop == SBE_TERM_APPEND_TRIPPED;  // the next step: a new term
        tail_got = tripped ? 64 : (std::size_t)r.appended.next;
        tail_exp = a.stop == SBE_TERM_APPEND_TRIPPED ? 64 : (std::size_t)a.next;
    }
    std::fclose(f);
    if (bad) return 1;
    std::printf("egress step host: ok\n");
    return 0;
}
