// TEST ONLY: a stand-alone host program over the piece location of sbe_term_poll's gather
// (csrc/term_poll_locate.hpp: tp_gather_from / tp_locate, which the kernel runs for entries of several
// fragments, under tp_find_msg / tp_gather, the serial form of the kernel's wave search and 64-entry
// rounds, which the GPU tests cover), built plain and with
// -fsanitize=address,undefined.  It reads the case files tests/termscan_lib.py writes (write_cases),
// walks every block with the host mirror's term_walk, reassembles the fragments serially as
// LocalFragmentReassembler::onFragment does (the expected bytes), builds the message tables as
// frag_scan_msgs defines them, and gathers the whole output through tp_gather in pieces of 64, 1024
// and kTpPiece bytes into a heap block of exactly the output's size, from a block and a carry held
// in heap blocks of exactly their sizes (so a read or write one byte outside is reported).  Every
// case runs without a carry and with carries of 1, 17, 1376 and 70 000 bytes.
// Exit status 0: every gather equalled the serial answer.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "aeron_cluster_amd.hpp"
#include "term_poll_locate.hpp"

template <class T>
static bool rd(FILE* f, std::vector<T>& v, std::uint64_t count) {
    v.resize(count);
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

struct Tables {
    std::vector<std::int64_t> frag_off;
    std::vector<std::uint8_t> flags;
    std::vector<std::uint32_t> src;  // ~0u: the carry
    std::vector<std::uint64_t> msg_off, msize, mfirst, mlast;
    std::vector<std::uint8_t> expect;  // the messages, then the open accumulator
};

static const std::uint32_t kFromCarry = 0xffffffffu;

static const std::uint8_t* frag_bytes(const Tables& t, const std::uint8_t* block, const std::uint8_t* carry, std::uint64_t f) {
    return t.src[f] == kFromCarry ? carry : block + t.src[f] + 32;
}

static Tables build(const aeron_cluster::TermFragments& w, const std::uint8_t* block, const std::uint8_t* carry,
                    std::uint64_t carry_bytes) {
    Tables t;
    if (carry_bytes) {
        t.frag_off.push_back(-(std::int64_t)carry_bytes);
        t.flags.push_back(0);
        t.src.push_back(kFromCarry);
    }
    for (std::size_t i = 0; i < w.flags.size(); ++i) {
        t.frag_off.push_back((std::int64_t)w.frag_off[i]);
        t.flags.push_back(w.flags[i]);
        t.src.push_back(w.frag_src[i]);
    }
    t.frag_off.push_back((std::int64_t)w.frag_off[w.flags.size()]);
    const std::uint64_t n = t.flags.size();
    std::vector<std::uint8_t> acc;
    std::int64_t lb = -1, le = -1;  // last BEGIN / END among the non-single fragments so far
    auto group = [&](std::uint64_t i, std::int64_t le_before, std::uint64_t& first, std::uint64_t& last) {
        std::int64_t s0 = lb > le_before + 1 ? lb : le_before + 1;
        if (s0 < 0) s0 = 0;
        bool gap = false;
        for (std::uint64_t f = (std::uint64_t)s0; f <= i && i < n; ++f) gap = gap || tp_single(t.flags[f]);
        first = (std::uint64_t)s0;
        last = i | (gap ? kTpGap : 0);
    };
    auto deliver = [&](const std::uint8_t* p, std::uint64_t len, std::uint64_t first, std::uint64_t last) {
        t.msg_off.push_back(t.expect.size());
        t.msize.push_back(len);
        t.mfirst.push_back(first);
        t.mlast.push_back(last);
        t.expect.insert(t.expect.end(), p, p + len);
    };
    for (std::uint64_t i = 0; i < n; ++i) {
        const std::uint8_t* p = frag_bytes(t, block, carry, i);
        const std::uint64_t len = (std::uint64_t)(t.frag_off[i + 1] - t.frag_off[i]);
        const std::uint8_t f = t.flags[i];
        if (tp_single(f)) {
            deliver(p, len, i, i);
            continue;
        }
        if (f & 0x80) {
            acc.clear();
            lb = (std::int64_t)i;
        }
        acc.insert(acc.end(), p, p + len);
        if (f & 0x40) {
            std::uint64_t first, last;
            group(i, le, first, last);
            deliver(acc.data(), acc.size(), first, last);
            acc.clear();
            le = (std::int64_t)i;
        }
    }
    std::uint64_t first = 0, last = 0;
    if (n) group(n - 1, le, first, last);
    deliver(acc.data(), acc.size(), first, last);  // entry m: the open accumulator
    return t;
}

struct HostCopy {
    const Tables& t;
    const std::uint8_t* block;
    const std::uint8_t* carry;
    std::uint8_t* out;
    std::uint64_t bytes = 0;
    void operator()(std::uint64_t pos, std::uint64_t f, std::uint64_t at, std::uint64_t n) {
        std::memcpy(out + pos, frag_bytes(t, block, carry, f) + at, n);
        bytes += n;
    }
};

static int run(const char* path, std::uint64_t& gathers) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    std::uint64_t count = 0;
    if (std::fread(&count, 8, 1, f) != 1) return 3;
    const std::uint64_t carries[] = {0, 1, 17, 1376, 70000};
    const std::uint64_t pieces[] = {64, 1024, kTpPiece};
    for (std::uint64_t k = 0; k < count; ++k) {
        std::uint64_t h[6];
        if (std::fread(h, 8, 6, f) != 6) return 3;
        std::vector<std::uint8_t> block, flags;
        std::vector<std::uint64_t> frag_off;
        std::vector<std::uint32_t> frag_src;
        if (!rd(f, block, h[0]) || !rd(f, frag_off, h[3] + 1) || !rd(f, frag_src, h[3]) || !rd(f, flags, h[3])) return 4;
        const aeron_cluster::TermFragments w = aeron_cluster::term_walk(block.data(), block.size(), h[1], h[2]);
        if (w.frag_off != frag_off || w.frag_src != frag_src || w.flags != flags) return 5;
        for (const std::uint64_t cb : carries) {
            std::vector<std::uint8_t> carry(cb);
            for (std::uint64_t i = 0; i < cb; ++i) carry[i] = (std::uint8_t)(0x5b + 7 * i + (i >> 7));
            const Tables t = build(w, block.data(), carry.data(), cb);
            const std::uint64_t m = t.msg_off.size() - 1, total = t.expect.size();
            const TpTables T{t.frag_off.data(), t.flags.data(), t.msg_off.data(), t.msize.data(), t.mfirst.data(),
                             t.mlast.data(), m};
            for (const std::uint64_t piece : pieces) {
                std::vector<std::uint8_t> out(total, 0xA5);
                HostCopy copy{t, block.data(), carry.data(), out.data()};
                for (std::uint64_t pos = 0; pos < total; pos += piece)
                    tp_gather(T, pos, total - pos < piece ? total : pos + piece, copy);
                ++gathers;
                if (copy.bytes != total || out != t.expect) {
                    std::fprintf(stderr, "case %llu, carry %llu, piece %llu: %llu of %llu bytes copied, %s\n",
                                 (unsigned long long)k, (unsigned long long)cb, (unsigned long long)piece,
                                 (unsigned long long)copy.bytes, (unsigned long long)total,
                                 out == t.expect ? "bytes equal" : "bytes differ");
                    return 6;
                }
            }
        }
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 64;
    std::uint64_t gathers = 0;
    for (int i = 1; i < argc; ++i) {
        const int rc = run(argv[i], gathers);
        if (rc) {
            std::fprintf(stderr, "%s: mismatch or bad file (%d)\n", argv[i], rc);
            return 1;
        }
    }
    std::printf("term poll locate: %llu gathers ok\n", (unsigned long long)gathers);
    return 0;
}
