// TEST ONLY: a stand-alone program over the host build of csrc/commit_fallback.hpp
// (fallback_host_check.cpp), meant to be linked with -fsanitize=address,undefined.  It reads case
// files written by tests/test_commit_fallback_ref.py, gives every array a heap block of exactly
// its size (so a read or write one byte outside it is reported), runs chk_emit_fb and compares
// with the expected outputs stored in the file.  Exit status 0: every case matched.
//
// File: 15 u64 {magic, n, k, data_bytes, flags, session, term, sess, cap, has_seq, has_mask,
// exp_out_bytes, default_ident_len, now_ns, uuid_ns}, then the arrays back to back in the order
// read below.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" int chk_emit_fb(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const uint8_t* status,
                           const uint8_t* flags, const uint32_t* view_off, const uint32_t* view_len,
                           const uint64_t* seq, const uint64_t* ts, const uint8_t* cm, const uint8_t* kind,
                           const uint32_t* tok_off, const uint32_t* tok_len, const uint32_t* tidx,
                           const uint64_t* last, const uint32_t* topic_id, const uint8_t* iarena,
                           const uint32_t* ioff, const uint8_t* tarena, const uint32_t* toff, uint32_t k,
                           const uint8_t* dident, uint32_t didentn, uint64_t now_ns, uint64_t uuid_ns,
                           const uint8_t* mask, uint32_t flg, int session, int64_t term, int64_t sess, uint8_t* out,
                           uint64_t cap, uint64_t* out_off, uint8_t* st, uint64_t* emit_idx, uint64_t* totals);

template <class T>
static bool rd(FILE* f, std::vector<T>& v, uint64_t count) {
    v.resize(count);
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

static int run(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    uint64_t h[15];
    if (std::fread(h, 8, 15, f) != 15 || h[0] != 0x3130424643544d43ull) return 3;
    const uint64_t n = h[1], k = h[2];
    std::vector<uint8_t> data, status, flags, cm, kind, iarena, tarena, dident, mask, exp_status, exp_out;
    std::vector<uint64_t> rec_off, seq, ts, last, exp_off, exp_idx, exp_tot;
    std::vector<uint32_t> view_off, view_len, tok_off, tok_len, tidx, topic_id, ioff, toff;
    bool ok = rd(f, data, h[3]) && rd(f, rec_off, n + 1) && rd(f, status, n) && rd(f, flags, n) &&
              rd(f, view_off, 5 * n) && rd(f, view_len, 5 * n) && rd(f, seq, h[9] ? n : 0) && rd(f, ts, n) &&
              rd(f, cm, n) && rd(f, kind, n) && rd(f, tok_off, n) && rd(f, tok_len, n) && rd(f, tidx, n) &&
              rd(f, last, k) && rd(f, topic_id, k) && rd(f, iarena, 4096) && rd(f, ioff, k + 1) &&
              rd(f, tarena, 4096) && rd(f, toff, k + 1) && rd(f, dident, h[12]) && rd(f, mask, h[10] ? n : 0) &&
              rd(f, exp_off, n + 1) && rd(f, exp_status, n) && rd(f, exp_tot, 3);
    ok = ok && rd(f, exp_idx, exp_tot[0]) && rd(f, exp_out, h[11]);
    std::fclose(f);
    if (!ok) return 4;
    std::vector<uint8_t> out(h[8]), st(n);
    std::vector<uint64_t> out_off(n + 1), idx(exp_tot[0]), tot(3);
    const int rc = chk_emit_fb(data.data(), rec_off.data(), n, status.data(), flags.data(), view_off.data(),
                               view_len.data(), h[9] ? seq.data() : nullptr, ts.data(), cm.data(), kind.data(),
                               tok_off.data(), tok_len.data(), tidx.data(), last.data(), topic_id.data(),
                               iarena.data(), ioff.data(), tarena.data(), toff.data(), (uint32_t)k, dident.data(),
                               (uint32_t)h[12], h[13], h[14], h[10] ? mask.data() : nullptr, (uint32_t)h[4],
                               (int)h[5], (int64_t)h[6], (int64_t)h[7], out.data(), h[8], out_off.data(), st.data(),
                               idx.data(), tot.data());
    if (rc != 0) return 5;
    if (out_off != exp_off || st != exp_status || idx != exp_idx || tot != exp_tot) return 6;
    if (exp_out.size() > out.size() || (exp_out.size() && std::memcmp(out.data(), exp_out.data(), exp_out.size()))) return 7;
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
