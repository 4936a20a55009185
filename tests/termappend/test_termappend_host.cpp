// TermAppender::append / append_batch (sbe_term_append on the device, the written bytes copied back)
// against the host mirror's term_append, over the case file of tests/termappend_lib.py (write_cases;
// the stored expectation is checked against term_append too) and over an encoded batch.  Both run
// on a block filled with 0xA5, so a byte either of them writes where the other does not shows.
// Prints one line per case ("case k: appended a next n stop s") and "term append host: ok" with exit
// status 0 when every result agrees.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "aeron_cluster_amd.hpp"
#include "sbecodec.h"

using namespace aeron_cluster;

template <class T>
static bool rd(FILE* f, std::vector<T>& v, std::uint64_t count) {
    v.resize(count);
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

int main(int argc, char** argv) {
    if (argc < 2) return 64;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::uint64_t count = 0;
    if (std::fread(&count, 8, 1, f) != 1) return 3;
    TermAppender dev;
    int bad = 0;
    for (std::uint64_t k = 0; k < count; ++k) {
        std::uint64_t h[11];
        std::int32_t id[5];
        if (std::fread(h, 8, 11, f) != 11 || std::fread(id, 4, 5, f) != 5) return 3;
        std::vector<std::uint8_t> in, expect;
        std::vector<std::uint64_t> rec_off, rec_tail;
        if (!rd(f, in, h[5]) || !rd(f, rec_off, h[6] + 1) || !rd(f, rec_tail, h[7]) || !rd(f, expect, h[0])) return 4;
        TermAppendOptions o;
        o.mtu = (std::uint32_t)h[3];
        o.limit = h[2];
        o.max_message_length = h[4];
        o.header = {id[0], id[1], id[2], id[3], (std::uint8_t)id[4]};
        std::vector<std::uint8_t> hb(h[0], 0xA5), db(h[0], 0xA5);
        const TermAppendResult hr = term_append(hb.data(), hb.size(), h[1], in.data(), in.size(), rec_off.data(), h[6], o);
        if (hb != expect || hr.appended != h[7] || hr.next != h[8] || hr.stop != h[10] || hr.rec_tail != rec_tail) {
            std::printf("case %llu: term_append differs from the stored expectation\n", (unsigned long long)k);
            ++bad;
        }
        const TermAppendResult dr = dev.append(in.data(), in.size(), rec_off.data(), h[6], db.data(), db.size(), h[1], o);
        const bool same = db == hb && dr.appended == hr.appended && dr.next == hr.next && dr.stop == hr.stop && dr.rec_tail == hr.rec_tail;
        std::printf("case %llu: appended %zu next %llu stop %u%s\n", (unsigned long long)k, dr.appended,
                    (unsigned long long)dr.next, dr.stop, same ? "" : "  DIFFERS from term_append");
        if (!same) ++bad;
    }
    std::fclose(f);
    // an encoded batch as the encoder leaves it, from its second record on, at an MTU that fragments
    {
        const std::string pay(300, 'p');
        const std::vector<TopicMessageFields> msgs = {{"t", "m", "u-0", "first", "{}", 1}, {"t", "m", "u-1", pay, "{}", 2},
                                                      {"t", "m", "u-2", "third", "{}", 3}};
        const EncodedBatch b = SBEEncoder::encode_topic_batch(msgs);
        TermAppendOptions o;
        o.mtu = 128;
        o.term_length = 1 << 20;  // the block is a part of a 1 MiB term: records up to 128 KiB
        o.header = {7, 1001, 3, 4096, 1};
        std::vector<std::uint8_t> hb(1024, 0xA5), db(1024, 0xA5);
        const TermAppendResult hr = term_append(hb.data(), hb.size(), 64, b.bytes.data(), b.bytes.size(), b.offsets.data() + 1, 2, o);
        const TermAppendResult dr = dev.append_batch(b, 1, db.data(), db.size(), 64, o);
        const bool same = db == hb && dr.appended == 2 && hr.appended == 2 && dr.next == hr.next && dr.stop == hr.stop &&
                          dr.rec_tail == hr.rec_tail;
        std::printf("batch: appended %zu next %llu stop %u%s\n", dr.appended, (unsigned long long)dr.next, dr.stop,
                    same ? "" : "  DIFFERS from term_append");
        if (!same) ++bad;
    }
    if (bad) return 1;
    std::printf("term append host: ok\n");
    return 0;
}
