// term_poll_locate.hpp — where the bytes of sbe_term_poll's output come from, as plain code over
// the call's tables.  Included by term_poll.hpp and by the host program of tests/termpoll;
// <stdint.h> comes first.  What the two share: tp_gather_from and tp_locate, the walk over an entry's
// fragments, which the gather kernel runs for every entry of several fragments.  tp_find_msg and
// tp_gather are the serial form of what the kernel does around that walk with the wave
// (tp_find_msg_wave, the 64-entry rounds of term_poll_gather and tp_copy_ones in term_poll.hpp, which
// only a device can run): the host program gathers whole outputs through them, the kernel does not
// call them.
//
// The tables (all in the call's workspace but msg_off, which is the caller's):
//   frag_off[f]   i64, n + 1 entries: the payloads' offsets as if they lay back to back, fragment f
//                 has frag_off[f + 1] - frag_off[f] bytes.  The walk's first payload is at 0; a
//                 carry is fragment 0 and lies in front of it, at -carry_bytes (only differences
//                 and order are used, so the tables of sbe_term_scan serve unchanged)
//   flags[f]      header byte 5 (the carry: 0, a middle fragment)
//   msg_off[j], msize[j], mfirst[j], mlast[j]   message j's place in out, its bytes, and the first
//                 and last fragment of its group; entry m is the open accumulator.  Bit 63 of
//                 mlast: a BEGIN|END single sits inside the group (it is a message of its own and
//                 no part of this one).  Without the bit the group's fragments are consecutive
// Where each fragment's bytes are (the block, or the carry buffer) is the caller's business: the
// walk hands runs of (output offset, fragment, offset in the fragment, bytes) to `copy`.
#ifndef TP_HD
#if defined(__HIPCC__)
#define TP_HD __host__ __device__ __forceinline__
#else
#define TP_HD inline
#endif
#endif

struct TpTables {
    const int64_t* frag_off;
    const uint8_t* flags;
    const uint64_t* msg_off;
    const uint64_t* msize;
    const uint64_t* mfirst;
    const uint64_t* mlast;
    uint64_t m;  // messages; entry m of the four message arrays is the open accumulator
};

constexpr uint64_t kTpGap = 1ull << 63;
constexpr uint32_t kTpPiece = 4096;  // bytes of output one wave of the gather copies (term_poll.hpp says why)

TP_HD bool tp_single(uint8_t f) { return (f & 0xC0u) == 0xC0u; }

// The entry j in [0, m] whose bytes hold output offset pos (pos < msg_off[m] + msize[m]): the last
// one that starts at or before pos (an empty message shares its offset with the one behind it).
TP_HD uint64_t tp_find_msg(const TpTables& T, uint64_t pos) {
    uint64_t lo = 0, hi = T.m;  // msg_off[lo] <= pos (msg_off[0] = 0); the answer lies in [lo, hi]
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (T.msg_off[mid] <= pos)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// Byte r (r < msize[j]) of entry j: its fragment f and the offset `at` in it.
TP_HD void tp_locate(const TpTables& T, uint64_t j, uint64_t r, uint64_t& f, uint64_t& at) {
    const uint64_t first = T.mfirst[j], ml = T.mlast[j], last = ml & ~kTpGap;
    if (!(ml & kTpGap)) {
        // consecutive fragments: byte r is at frag_off[first] + r of the back-to-back payloads; the
        // last fragment that starts at or before it holds it (empty ones share its offset)
        const int64_t key = T.frag_off[first] + (int64_t)r;
        uint64_t lo = first, hi = last;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (T.frag_off[mid] <= key)
                lo = mid;
            else
                hi = mid - 1;
        }
        f = lo;
        at = (uint64_t)(key - T.frag_off[lo]);
        return;
    }
    // singles inside the group: their bytes lie between the group's in frag_off, so count the
    // group's own bytes from its first fragment.  A known limit: linear in the group's fragments,
    // a dependent load a step, repeated by every piece of the message (a 16 MiB message with one
    // single inside: 12 000 steps in each of 4096 waves).  Nothing bounds such groups; a
    // publication does not interleave its own messages, so only a malformed stream has them.
    uint64_t acc = 0;
    for (f = first; f < last; ++f) {
        if (tp_single(T.flags[f])) continue;
        const uint64_t len = (uint64_t)(T.frag_off[f + 1] - T.frag_off[f]);
        if (acc + len > r) break;
        acc += len;
    }
    at = r - acc;
}

// The output bytes [pos, end) (end <= msg_off[m] + msize[m]) as runs: copy(out offset, fragment,
// offset in the fragment, bytes), in output order, every byte exactly once.
// j: the entry that holds pos (tp_find_msg's answer).
template <class Copy>
TP_HD void tp_gather_from(const TpTables& T, uint64_t j, uint64_t pos, uint64_t end, Copy& copy) {
    if (pos >= end) return;
    uint64_t f, at;
    uint64_t rest = T.msize[j] - (pos - T.msg_off[j]);  // of entry j, from pos on
    uint64_t ml = T.mlast[j];
    tp_locate(T, j, pos - T.msg_off[j], f, at);
    while (pos < end) {
        if (rest == 0) {  // the next entry (pos < end: there is one), from its first fragment
            if (++j > T.m) return;
            rest = T.msize[j];
            ml = T.mlast[j];
            f = T.mfirst[j];
            at = 0;
            continue;
        }
        if (f > (ml & ~kTpGap)) return;  // never with tables of this library: stay inside them
        if ((ml & kTpGap) && tp_single(T.flags[f])) {
            ++f;
            continue;
        }
        const uint64_t len = (uint64_t)(T.frag_off[f + 1] - T.frag_off[f]);
        if (at >= len) {
            ++f;
            at = 0;
            continue;
        }
        uint64_t n = len - at;
        n = n < rest ? n : rest;
        n = n < end - pos ? n : end - pos;
        copy(pos, f, at, n);
        pos += n;
        at += n;
        rest -= n;
    }
}

template <class Copy>
TP_HD void tp_gather(const TpTables& T, uint64_t pos, uint64_t end, Copy& copy) {
    if (pos < end) tp_gather_from(T, tp_find_msg(T, pos), pos, end, copy);
}
