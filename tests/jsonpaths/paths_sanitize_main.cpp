// TEST ONLY: a stand-alone program over the host build of csrc/json_paths.hpp
// (paths_host_check.cpp), meant to be linked with -fsanitize=address,undefined.  It reads case
// files written by tests/test_jsonpaths_ref.py and runs chk_extract record by record, each record
// in a heap block of exactly its size and each output row in one of exactly P entries (so a read
// or write one byte outside them is reported), then compares with the expected outputs stored in
// the file.  Exit status 0: every case matched.
//
// File: 8 u64 {magic, n, data_bytes, has_dec, view, has_select, n_paths, n_names}, then the arrays
// back to back in the order read below.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" int chk_extract(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const uint8_t* status,
                           const uint8_t* flags, const uint32_t* view_off, const uint32_t* view_len, uint32_t view,
                           const uint8_t* select, uint32_t n_paths, const uint8_t* depth, const uint8_t* names,
                           const uint32_t* name_off, uint8_t* doc, uint8_t* root_kind, uint8_t* kind, uint32_t* off,
                           uint32_t* len);

template <class T>
static bool rd(FILE* f, std::vector<T>& v, uint64_t count) {
    v.resize(count);
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

static int run(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    uint64_t h[8];
    if (std::fread(h, 8, 8, f) != 8 || h[0] != 0x3130485441504a53ull) return 3;
    const uint64_t n = h[1], P = h[6];
    const bool has_dec = h[3] != 0, has_sel = h[5] != 0;
    std::vector<uint8_t> data, status, flags, select, depth, names, exp_doc, exp_root, exp_kind;
    std::vector<uint64_t> rec_off;
    std::vector<uint32_t> view_off, view_len, name_off, exp_off, exp_len;
    bool ok = rd(f, data, h[2]) && rd(f, rec_off, n + 1) && rd(f, status, has_dec ? n : 0) &&
              rd(f, flags, has_dec ? n : 0) && rd(f, view_off, has_dec ? 5 * n : 0) &&
              rd(f, view_len, has_dec ? 5 * n : 0) && rd(f, select, has_sel ? n : 0) && rd(f, depth, P) &&
              rd(f, name_off, h[7] + 1);
    ok = ok && rd(f, names, name_off[h[7]]) && rd(f, exp_doc, n) && rd(f, exp_root, n) && rd(f, exp_kind, n * P) &&
         rd(f, exp_off, n * P) && rd(f, exp_len, n * P);
    std::fclose(f);
    if (!ok) return 4;
    for (uint64_t i = 0; i < n; ++i) {
        const std::vector<uint8_t> rec(data.begin() + rec_off[i], data.begin() + rec_off[i + 1]);
        const uint64_t ro[2] = {0, rec.size()};
        std::vector<uint8_t> doc(1), root(1), kind(P);
        std::vector<uint32_t> off(P), len(P);
        const int rc = chk_extract(rec.data(), ro, 1, has_dec ? &status[i] : nullptr, has_dec ? &flags[i] : nullptr,
                                   has_dec ? &view_off[5 * i] : nullptr, has_dec ? &view_len[5 * i] : nullptr,
                                   (uint32_t)h[4], has_sel ? &select[i] : nullptr, (uint32_t)P, depth.data(),
                                   names.data(), name_off.data(), doc.data(), root.data(), kind.data(), off.data(),
                                   len.data());
        if (rc != 0) return 5;
        if (doc[0] != exp_doc[i] || root[0] != exp_root[i]) return 6;
        if (std::memcmp(kind.data(), &exp_kind[i * P], P) || std::memcmp(off.data(), &exp_off[i * P], 4 * P) ||
            std::memcmp(len.data(), &exp_len[i * P], 4 * P))
            return 7;
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
