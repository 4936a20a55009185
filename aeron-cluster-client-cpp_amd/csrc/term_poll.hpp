// term_poll.hpp — included by sbe_codec.hip inside its anonymous namespace, after term_scan.hpp.
//
// sbe_term_poll: sbe_term_scan's walk and sbe_reassemble_fragments in one call, with the fragment
// count handed on in device memory and every payload byte copied once, from the block (or the carry
// buffer) straight into its message.
//
//   tables          term_tile_chain / term_walk_tiles / term_emit as they are, with out == NULL:
//                   frag_off / flags / frag_src go to the workspace, counts[0..3] to the caller.
//                   With a carry the three tables start at entry 1 and tp_carry_entry writes entry
//                   0: carry_bytes long, flags 0 (a middle fragment appends exactly as the
//                   accumulator would), source kTpFromCarry.  frag_off is read as i64 from here on:
//                   the walk's first payload is at 0, the carry in front of it at -carry_bytes
//   scan            frag_reduce / frag_scan_blocks / frag_scan_msgs (their bodies) from kernels that
//                   read n = counts[0] (+ 1 with a carry) first: the grids are sized from the
//                   capacity and a block past n leaves.  counts[0] is complete only after term_emit
//                   (a LIMIT stop writes it there).  frag_scan_msgs writes {m, carry} to counts[4..5]
//   term_poll_gather  output-first, as ta_write on the publish side: the output [0, msg_off[m] +
//                   carry) in pieces of kTpPiece bytes, one wave a piece.  The wave finds the
//                   piece's message by a search in msg_off (tp_find_msg_wave) and takes the entries
//                   from there 64 at a time: one-fragment messages are copied together
//                   (tp_copy_ones); for an entry of several fragments tp_gather_from
//                   (term_poll_locate.hpp, shared with the host program of tests/termpoll) finds the
//                   first fragment by a search in frag_off and walks the fragments forward, the wave
//                   copying each run with wave_copy16.  Payloads in a block are never back to
//                   back (a header and the alignment tail lie between any two), so there are no runs
//                   of fragments to copy as one, and a per-message wave would copy a 16 MiB message
//                   in 12 000 steps: cut by output bytes, a long message spreads over the grid with
//                   no list of long messages, and short ones cost one search a piece, not one each.

#include "term_poll_locate.hpp"

// One piece is one full step of wave_copy16 (kFcU chunks of 16 bytes a lane): a smaller one leaves
// lanes idle on contiguous bytes, a larger one puts more 1376-byte fragments (a run each, with a
// byte-wise head and tail) behind each other in one wave while others have nothing to do.  A 16 MiB
// block is 4096 pieces, one wave each on 256 CUs; the search a piece (three rounds of 64 probes for
// 46 000 messages) is shared by about three 1376-byte fragments or fourteen 300-byte messages.
static_assert(kTpPiece == 16u * kFcU * kWave, "kTpPiece (term_poll_locate.hpp) is one step of wave_copy16");
constexpr uint32_t kTpFromCarry = 0xffffffffu;  // frag_src of the carry entry (a block has at most 2^30 bytes)
constexpr uint32_t kTpWaves = 4;                // waves (pieces) per workgroup of the gather

struct TpArgs {
    const uint8_t* block;
    const uint8_t* carry;
    uint8_t* out;
    const uint32_t* frag_src;
    TpTables T;              // T.m is read from counts in the kernel
    const uint64_t* counts;  // the caller's six
};

__global__ void tp_carry_entry(int64_t* frag_off, uint8_t* flags, uint32_t* frag_src, uint64_t carry_bytes) {
    frag_off[0] = -(int64_t)carry_bytes;
    flags[0] = 0;
    frag_src[0] = kTpFromCarry;
}

// n of the reassembly: the delivered fragments, and the carry entry in front of them
__device__ __forceinline__ uint64_t tp_n(const uint64_t* counts, uint32_t lead) { return counts[0] + lead; }

__global__ __launch_bounds__(kFsThreads) void tp_frag_reduce(FragArgs a, FragScan* agg, const uint64_t* counts, uint32_t lead) {
    a.n = tp_n(counts, lead);
    if ((uint64_t)blockIdx.x * kFsBlk >= a.n) return;
    frag_reduce_body(a, agg);
}

// msg_off / counts4 are written here when there is no fragment at all (frag_scan_msgs writes them
// from the last fragment's thread)
__global__ __launch_bounds__(kFsbThreads) void tp_frag_scan_blocks(FragScan* agg, const uint64_t* counts, uint32_t lead,
                                                                   uint64_t* msg_off, uint64_t* counts4) {
    const uint64_t n = tp_n(counts, lead);
    if (n == 0) {
        if (threadIdx.x == 0) {
            msg_off[0] = 0;
            counts4[0] = 0;
            counts4[1] = 0;
        }
        return;
    }
    frag_scan_blocks_body(agg, (n + kFsBlk - 1) / kFsBlk, nullptr);
}

__global__ __launch_bounds__(kFsThreads) void tp_frag_scan_msgs(FragArgs a, const FragScan* pre, const uint64_t* counts,
                                                                uint32_t lead) {
    a.n = tp_n(counts, lead);
    if ((uint64_t)blockIdx.x * kFsBlk >= a.n) return;
    frag_scan_msgs_body(a, pre);
}

struct TpWaveCopy {
    const TpArgs& a;
    int lane;
    __device__ __forceinline__ void operator()(uint64_t pos, uint64_t f, uint64_t at, uint64_t n) const {
        const uint32_t src = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.frag_src[f]);
        // in the block: behind the frame's 32-byte header (32-byte aligned; the carry has no alignment)
        const uint8_t* from = src == kTpFromCarry ? a.carry : a.block + src + 32;
        wave_copy16(a.out + uniform64(pos), from + uniform64(at), uniform64(n), lane);
    }
};

// tp_find_msg with the wave: 64 probes a round instead of one (three dependent loads for 46 000
// messages where the binary search takes sixteen); the same answer.
__device__ __forceinline__ uint64_t tp_find_msg_wave(const uint64_t* msg_off, uint64_t m, uint64_t pos, int lane) {
    uint64_t lo = 0, hi = m;  // msg_off[lo] <= pos; the answer lies in [lo, hi]
    while (hi - lo >= (uint64_t)kWave) {
        const uint64_t step = (hi - lo) / kWave + 1, idx = lo + ((uint64_t)lane + 1) * step;
        const int k = __popcll(__ballot(idx <= hi && msg_off[idx] <= pos));  // msg_off ascends: the first k probes
        const uint64_t top = lo + ((uint64_t)k + 1) * step - 1;
        lo += (uint64_t)k * step;
        hi = top < hi ? top : hi;
    }
    const uint64_t idx = lo + (uint64_t)lane;
    return lo + (uint64_t)__popcll(__ballot(idx <= hi && msg_off[idx] <= pos)) - 1;  // lane 0 always counts
}

// Up to 64 short copies at once, one a lane (len 0: none; the lens add up to kTpPiece at the most):
// dst[0, len) = src[0, len).  Each lane writes its own copy's bytes in front of the first 16-byte
// boundary of dst and behind the last; the 16-byte chunks between them, of all the copies together,
// are numbered through (a wave scan) and dealt to the lanes, which find their chunk's copy by a
// search in the scan, so a 300-byte message's 18 chunks do not leave 46 lanes idle and fourteen
// messages do not wait for one another (copied one after the other with wave_copy16 they did:
// DESIGN §5).  Loads at any byte address, aligned nontemporal stores, as wave_copy16.
__device__ __forceinline__ void tp_copy_ones(uint8_t* dst, const uint8_t* src, uint32_t len, int lane) {
    uint32_t head = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
    head = head < len ? head : len;
    const uint32_t nc = (len - head) >> 4, t0 = head + 16u * nc, tail = len - t0;
#pragma unroll
    for (uint32_t b = 0; b < 15; ++b)
        if (b < head) dst[b] = src[b];
#pragma unroll
    for (uint32_t b = 0; b < 15; ++b)
        if (b < tail) dst[t0 + b] = src[t0 + b];
    const uint32_t incl = (uint32_t)wave_incl_scan64(nc, lane), excl = incl - nc;
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
    const uintptr_t d = reinterpret_cast<uintptr_t>(dst) + head, s = reinterpret_cast<uintptr_t>(src) + head;
    for (uint32_t c0 = 0; c0 < total; c0 += kFcU * kWave) {
        uint4 x[kFcU];
        uintptr_t to[kFcU];
#pragma unroll
        for (int u = 0; u < kFcU; ++u) {
            const uint32_t c = c0 + (uint32_t)lane + (uint32_t)kWave * u;
            uint32_t e = 0;  // the copies that end at or before chunk c: the index of c's copy
#pragma unroll
            for (uint32_t step = kWave / 2; step; step >>= 1)
                if ((uint32_t)__shfl((int)incl, (int)(e + step - 1), kWave) <= c) e += step;
            const uint64_t at = 16ull * (c - (uint32_t)__shfl((int)excl, (int)e, kWave));
            const uintptr_t from = (uintptr_t)__shfl((unsigned long long)s, (int)e, kWave) + at;
            to[u] = (uintptr_t)__shfl((unsigned long long)d, (int)e, kWave) + at;
            x[u] = make_uint4(0, 0, 0, 0);
            if (c < total) x[u] = gload128_ua(from);
        }
#pragma unroll
        for (int u = 0; u < kFcU; ++u) {
            const uint32_t c = c0 + (uint32_t)lane + (uint32_t)kWave * u;
            if (c < total) {
                u32x4 v;
                v.x = x[u].x, v.y = x[u].y, v.z = x[u].z, v.w = x[u].w;
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(to[u]));
            }
        }
    }
}

// One wave a piece.  The piece's entries 64 at a time, one a lane: an entry that is one fragment (a
// BEGIN|END single: nearly every message of an order stream) needs its table row and its fragment's
// source, loaded by all lanes at once, and the wave copies the entries' parts of the piece together
// (tp_copy_ones); an entry of several fragments goes through tp_gather_from.  (Walking every entry
// through tp_gather cost four dependent loads an entry, fourteen entries a piece of 300-byte
// messages: DESIGN §5.)
__global__ __launch_bounds__(kTpWaves* kWave) void term_poll_gather(TpArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    a.T.m = uniform64(a.counts[4]);
    const uint64_t total = uniform64(a.T.msg_off[a.T.m] + a.counts[5]);
    const uint64_t pos = ((uint64_t)blockIdx.x * kTpWaves + threadIdx.x / kWave) * kTpPiece;
    if (pos >= total) return;
    const uint64_t end = total - pos < kTpPiece ? total : pos + kTpPiece;
    TpWaveCopy copy{a, lane};
    for (uint64_t jb = tp_find_msg_wave(a.T.msg_off, a.T.m, pos, lane);; jb += kWave) {
        const uint64_t j = jb + (uint64_t)lane;
        const bool valid = j <= a.T.m;
        uint64_t mo = 0, sz = 0, mf = 0, ml = 0;
        if (valid) {
            mo = a.T.msg_off[j];
            sz = a.T.msize[j];
            mf = a.T.mfirst[j];
            ml = a.T.mlast[j];
        }
        const bool in = valid && sz > 0 && mo < end && mo + sz > pos;
        const bool one = in && mf == ml;  // one fragment, and no single-inside bit
        const uint32_t src = one ? a.frag_src[mf] : 0u;
        const uint64_t d0 = mo > pos ? mo : pos, d1 = mo + sz < end ? mo + sz : end;
        tp_copy_ones(a.out + d0, (src == kTpFromCarry ? a.carry : a.block + src + 32) + (d0 - mo),
                     one ? (uint32_t)(d1 - d0) : 0u, lane);
        for (uint64_t mk = __ballot(in && !one); mk; mk &= mk - 1) {
            const int k = __builtin_ctzll(mk);
            tp_gather_from(a.T, jb + (uint64_t)k, uniform64(__shfl(d0, k, kWave)), uniform64(__shfl(d1, k, kWave)), copy);
        }
        if (__ballot(!valid || mo >= end)) break;  // the piece ends among these entries, or the tables do
    }
}

// A call that delivers nothing (limit 0, or start == block_bytes): the six counts and msg_off[0];
// the carry goes out unchanged (tp_copy_carry).
__global__ void tp_counts_only(uint64_t* counts, uint64_t* msg_off, uint64_t next, uint32_t stop, uint64_t carry_bytes) {
    counts[0] = 0;
    counts[1] = next;
    counts[2] = 0;
    counts[3] = stop;
    counts[4] = 0;
    counts[5] = carry_bytes;
    msg_off[0] = 0;
}

__global__ __launch_bounds__(kTpWaves* kWave) void tp_copy_carry(uint8_t* out, const uint8_t* carry, uint64_t carry_bytes) {
    const uint64_t pos = ((uint64_t)blockIdx.x * kTpWaves + threadIdx.x / kWave) * kTpPiece;
    if (pos >= carry_bytes) return;
    wave_copy16(out + pos, carry + pos, carry_bytes - pos < kTpPiece ? carry_bytes - pos : kTpPiece,
                (int)(threadIdx.x & (kWave - 1)));
}
