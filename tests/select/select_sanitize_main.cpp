// TEST ONLY: a stand-alone program over the host build of csrc/order_select.hpp
// (select_host_check.cpp), meant to be linked with -fsanitize=address,undefined.  It reads case
// files written by tests/test_select_lib.py and runs chk_select twice: over the whole batch in a
// heap block of exactly its size, and record by record, each record in a heap block of exactly its
// size and each output in one of exactly one element (so a read or write one byte outside them is
// reported); both with the window and alignment the file names and with the smallest window.  It
// compares with the expected outputs stored in the file.  Exit status 0: every case matched.
//
// File: 5 u64 {magic, n, data_bytes, window, base_lead}, then data, rec_off [n + 1], status, flags,
// hdr [4 n], view_off [5 n], view_len [5 n], pred, select, topic_class.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" int chk_select(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const uint8_t* status,
                          const uint8_t* flags, const uint16_t* hdr, const uint32_t* view_off, const uint32_t* view_len,
                          uint32_t window, uint32_t base_lead, uint8_t* pred, uint8_t* select, uint8_t* topic_class,
                          uint64_t* totals);

template <class T>
static bool rd(FILE* f, std::vector<T>& v, uint64_t count) {
    v.resize(count);
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

static int run(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    uint64_t h[5];
    if (std::fread(h, 8, 5, f) != 5 || h[0] != 0x31304c45534f4253ull) return 3;
    const uint64_t n = h[1];
    std::vector<uint8_t> data, status, flags, exp_pred, exp_sel, exp_cls;
    std::vector<uint64_t> rec_off;
    std::vector<uint16_t> hdr;
    std::vector<uint32_t> view_off, view_len;
    const bool ok = rd(f, data, h[2]) && rd(f, rec_off, n + 1) && rd(f, status, n) && rd(f, flags, n) && rd(f, hdr, 4 * n) &&
                    rd(f, view_off, 5 * n) && rd(f, view_len, 5 * n) && rd(f, exp_pred, n) && rd(f, exp_sel, n) &&
                    rd(f, exp_cls, n);
    std::fclose(f);
    if (!ok) return 4;
    const uint32_t windows[2] = {(uint32_t)h[3], 48};
    for (uint32_t window : windows) {
        std::vector<uint8_t> pred(n), sel(n), cls(n);
        uint64_t totals[2];
        if (chk_select(data.data(), rec_off.data(), n, status.data(), flags.data(), hdr.data(), view_off.data(),
                       view_len.data(), window, (uint32_t)h[4], pred.data(), sel.data(), cls.data(), totals))
            return 5;
        if (pred != exp_pred || sel != exp_sel || cls != exp_cls) return 6;
        for (uint64_t i = 0; i < n; ++i) {
            const std::vector<uint8_t> rec(data.begin() + rec_off[i], data.begin() + rec_off[i + 1]);
            const uint64_t ro[2] = {0, rec.size()};
            std::vector<uint8_t> p(1), s(1), c(1);
            if (chk_select(rec.data(), ro, 1, &status[i], &flags[i], &hdr[4 * i], &view_off[5 * i], &view_len[5 * i], window,
                           (uint32_t)((h[4] + rec_off[i]) & 15), p.data(), s.data(), c.data(), totals))
                return 7;
            if (p[0] != exp_pred[i] || s[0] != exp_sel[i] || c[0] != exp_cls[i]) return 8;
            if (totals[0] != s[0] || totals[1] != ((p[0] & 8) ? 1u : 0u)) return 9;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 64;
    for (int i = 1; i < argc; ++i) {
        const int rc = run(argv[i]);
        if (rc) {
            std::fprintf(stderr, "%s: mismatch or bad file (%d)\n", argv[i], rc);
            return 1;
        }
    }
    std::printf("%d cases ok\n", argc - 1);
    return 0;
}
