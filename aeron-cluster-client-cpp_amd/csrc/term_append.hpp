// term_append.hpp — included by sbe_codec.hip inside its anonymous namespace, after term_scan.hpp.
//
// The mirror of term_scan.hpp: what an exclusive publication's offer loop writes into a term
// (ExclusiveTermAppender::appendUnfragmentedMessage / appendFragmentedMessage /
// handleEndOfLogCondition), for a whole batch of encoded records on the device (sbe_term_append).
// The frames of record i occupy required(L_i) bytes of the block, a pure function of its length, so
// the tails are an exclusive scan, and every stop condition holds from some first record onward.
//
//   ta_sums         one workgroup per kTaBlk records: required(L_i) of every well-formed record that
//                   is not too long (0 for the others: nothing behind the first of them is appended),
//                   the block's sum and the block's first such record (mat_block_scan, the
//                   materialize path's block scan)
//   ta_scan_blocks  one workgroup: the exclusive scan of the block sums in place, and the first
//                   record of the batch that is malformed or too long
//   ta_tails        one thread a record (and one behind the last): its tail from the block's base
//                   and the block scan; whether it stops the call (it is malformed or too long, its
//                   tail lies at or behind the limit, its frames run past the block) and whether the
//                   record before it does; the one thread whose record is the first to stop writes
//                   counts and the plan (how far the frames reach, where a padding header goes)
//   ta_write        output-driven: one workgroup per kTaTile bytes of block.  The tile's first record
//                   comes from a 64-ary search of the tails (64 probes a step, so three dependent
//                   loads for 46 k records where a binary search takes sixteen); the tails and source
//                   offsets of the tile's records are staged in LDS.  A lane composes aligned 16-byte
//                   chunks, four of them.  A chunk finds its record by a search of the staged tails,
//                   its frame by a division by the MTU, and is a header half, 16 payload bytes (one
//                   unaligned 16-byte load, the bytes behind the payload's end masked to the
//                   alignment zeros) or half of the padding-frame header: one decision per chunk,
//                   every byte of [start, next) stored once, 16 bytes a store

constexpr uint32_t kTaBlk = kMatBlk;            // records per plan workgroup (mat_block_scan's block)
constexpr uint32_t kTaThreads = 256;
constexpr uint32_t kTaTile = 16384;             // bytes of block per write workgroup: four chunks a lane
constexpr uint32_t kTaTileRecs = kTaTile / 32;  // a record takes at least one 32-byte frame
constexpr uint64_t kTaMaxBlock = 1ull << 30;
constexpr uint64_t kTaNone = ~0ull;

struct TaPlan {
    uint64_t first_static;  // the first malformed or too-long record, or kTaNone (ta_scan_blocks)
    uint64_t appended;
    uint64_t data_end;      // the frames of the appended records are block[start, data_end)
    uint64_t pad;           // 1: a padding-frame header goes to data_end
};

struct TaArgs {
    const uint8_t* in;
    uint64_t in_bytes;
    const uint64_t* rec_off;
    uint64_t n;
    uint8_t* block;
    uint64_t block_bytes;
    uint64_t start;
    uint64_t limit;
    uint32_t mtu;
    uint64_t max_len;
    sbe_term_header hdr;
    uint64_t* tails;   // [n] the caller's rec_tail, or workspace
    uint64_t* counts;
    uint64_t* bsum;    // [blocks] per plan workgroup: bytes of frames, then (in place) their exclusive scan
    uint64_t* bmin;    // [blocks] the first malformed or too-long record of each, or kTaNone
    TaPlan* plan;
};

__host__ __device__ __forceinline__ uint64_t ta_required(uint64_t L, uint32_t mtu) {
    const uint64_t maxp = mtu - 32u;
    if (L <= maxp) return (32 + L + 31) & ~31ull;
    const uint64_t rem = L % maxp;
    return (L / maxp) * mtu + (rem ? (32 + rem + 31) & ~31ull : 0);
}

struct TaRec {
    uint64_t len;
    bool bad, too_long;
    uint64_t req;  // 0 for a record that is bad or too long
};
// kIdx (sbe_term_append_counted): record i is rec_off[idx.at[i]] .. rec_off[idx.at[i] + 1] where
// idx.at is not null; an index at or past the capacity (rec_off has capacity + 1 entries) is a bad record
struct TaIdx {
    const uint64_t* at;  // [capacity] or nullptr
    uint64_t cap;
};
template <bool kIdx>
__device__ __forceinline__ uint64_t ta_src(const TaIdx& idx, uint64_t i) {
    return kIdx && idx.at ? idx.at[i] : i;
}
template <bool kIdx>
__device__ __forceinline__ TaRec ta_rec(const TaArgs& a, const TaIdx& idx, uint64_t i) {
    TaRec r{0, false, false, 0};
    if (i >= a.n) return r;
    const uint64_t s = ta_src<kIdx>(idx, i);
    if (kIdx && s >= idx.cap) {
        r.bad = true;
        return r;
    }
    const uint64_t lo = a.rec_off[s], hi = a.rec_off[s + 1];
    r.bad = hi < lo || hi > a.in_bytes;
    if (r.bad) return r;
    r.len = hi - lo;
    r.too_long = r.len > a.max_len;
    if (!r.too_long) r.req = ta_required(r.len, a.mtu);
    return r;
}

// minimum over the kTaBlk-thread block
__device__ __forceinline__ uint64_t ta_block_min(uint64_t v) {
    __shared__ uint64_t wm[kTaBlk / kWave];
    v = mat_wave_min(v);
    if ((threadIdx.x & (kWave - 1)) == 0) wm[threadIdx.x / kWave] = v;
    __syncthreads();
    uint64_t m = kTaNone;
#pragma unroll
    for (uint32_t k = 0; k < kTaBlk / kWave; ++k) m = wm[k] < m ? wm[k] : m;
    __syncthreads();
    return m;
}

template <bool kIdx>
__device__ __forceinline__ void ta_sums_block(const TaArgs& a, const TaIdx& idx) {
    const uint64_t i = (uint64_t)blockIdx.x * kTaBlk + threadIdx.x;
    const TaRec r = ta_rec<kIdx>(a, idx, i);
    uint64_t tot;
    (void)mat_block_scan(r.req, tot);
    const uint64_t m = ta_block_min((r.bad || r.too_long) ? i : kTaNone);
    if (threadIdx.x == 0) {
        a.bsum[blockIdx.x] = tot;
        a.bmin[blockIdx.x] = m;
    }
}
__global__ __launch_bounds__(kTaBlk) void ta_sums(TaArgs a) { ta_sums_block<false>(a, TaIdx{}); }

__global__ __launch_bounds__(kTaBlk) void ta_scan_blocks(TaArgs a, uint64_t nb) {
    uint64_t carry = 0, m = kTaNone;
    for (uint64_t c0 = 0; c0 < nb; c0 += kTaBlk) {
        const uint64_t j = c0 + threadIdx.x;
        uint64_t tot;
        const uint64_t v = j < nb ? a.bsum[j] : 0ull;
        const uint64_t f = j < nb ? a.bmin[j] : kTaNone;
        m = f < m ? f : m;
        const uint64_t ex = mat_block_scan(v, tot);
        __syncthreads();
        if (j < nb) a.bsum[j] = carry + ex;
        carry += tot;
        __syncthreads();
    }
    m = ta_block_min(m);
    if (threadIdx.x == 0) a.plan->first_static = m;
}

template <bool kIdx>
__device__ __forceinline__ void ta_tails_block(const TaArgs& a, const TaIdx& idx) {
    const uint64_t i = (uint64_t)blockIdx.x * kTaBlk + threadIdx.x;
    const TaRec r = ta_rec<kIdx>(a, idx, i);
    uint64_t tot;
    const uint64_t tb = a.start + a.bsum[blockIdx.x] + mat_block_scan(r.req, tot);  // the tail before record i
    if (kIdx && idx.at) {
        // the payload bytes: gathered records do not lie back to back, so the appended ones (those that
        // no stop condition holds for) add their lengths up, one atomic a wave (ta_sums_counted zeroed it)
        const uint64_t fs0 = a.plan->first_static;
        const bool in = i < a.n && i < fs0 && tb < a.limit && tb + r.req <= a.block_bytes;
        const uint64_t w = wave_sum64(in ? r.len : 0ull);
        if ((threadIdx.x & (kWave - 1)) == 0 && w) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts + 2), (unsigned long long)w);
    }
    if (i > a.n) return;
    if (i < a.n) a.tails[i] = tb + r.req;
    const uint64_t fs = a.plan->first_static;
    // every condition holds from its first record onward (the tail only grows), so the first record
    // that stops the call is the one that fails while the record before it does not
    const bool fails = i == a.n || i >= fs || tb >= a.limit || tb + r.req > a.block_bytes;
    bool prev = false;
    if (i > 0) {
        const TaRec p = ta_rec<kIdx>(a, idx, i - 1);
        prev = i - 1 >= fs || tb - p.req >= a.limit || tb > a.block_bytes;
    }
    if (!fails || prev) return;
    uint32_t stop = SBE_TERM_APPEND_TRIPPED;
    if (i == a.n) stop = SBE_TERM_APPEND_END;
    else if (r.bad) stop = SBE_TERM_APPEND_BAD_RECORD;
    else if (tb >= a.limit) stop = SBE_TERM_APPEND_LIMIT;
    else if (r.too_long) stop = SBE_TERM_APPEND_TOO_LONG;
    const bool trip = stop == SBE_TERM_APPEND_TRIPPED;
    a.plan->appended = i;
    a.plan->data_end = tb;
    a.plan->pad = trip && tb < a.block_bytes ? 1u : 0u;
    a.counts[0] = i;
    a.counts[1] = trip ? a.block_bytes : tb;
    if (!(kIdx && idx.at))
        a.counts[2] = a.rec_off[i] - a.rec_off[0];  // records 0..i-1 are well formed: the offsets up to i only grow
    a.counts[3] = stop;
}
__global__ __launch_bounds__(kTaBlk) void ta_tails(TaArgs a) { ta_tails_block<false>(a, TaIdx{}); }

// 16 bytes of `in` from byte s on, of which the first v (1..16) are payload: the others are zero.
// One unaligned load where all 16 lie inside `in`, bytewise at the very end of it.
__device__ __forceinline__ u32x4 ta_payload(const TaArgs& a, uint64_t s, uint32_t v) {
    u32x4 x;
    if (s + 16 <= a.in_bytes) {
        const uint4 t = gload128_ua(reinterpret_cast<uintptr_t>(a.in) + s);
        x.x = t.x & byte_mask_bits(v);
        x.y = v > 4 ? t.y & byte_mask_bits(v - 4) : 0u;
        x.z = v > 8 ? t.z & byte_mask_bits(v - 8) : 0u;
        x.w = v > 12 ? t.w & byte_mask_bits(v - 12) : 0u;
        return x;
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (uint32_t b = 0; b < v; ++b) w[b >> 2] |= (uint32_t)a.in[s + b] << (8 * (b & 3));
    x.x = w[0], x.y = w[1], x.z = w[2], x.w = w[3];
    return x;
}

template <bool kIdx>
__device__ __forceinline__ void ta_write_tile(const TaArgs& a, const TaIdx& idx, uint32_t tile0) {
    __shared__ uint32_t tail[kTaTileRecs + 2];  // tail[0]: the tail before the tile's first record; tail[k + 1]: behind record first + k
    __shared__ uint64_t src[kTaTileRecs + 2];   // rec_off[first + k]
    __shared__ uint32_t slen[kIdx ? kTaTileRecs + 2 : 1];  // kIdx: the record's length (its neighbour's start says nothing)
    const uint64_t appended = a.plan->appended, data_end = a.plan->data_end;
    const uint64_t t0 = (uint64_t)(tile0 + blockIdx.x) * kTaTile;
    const uint64_t lo = t0 > a.start ? t0 : a.start;
    const uint64_t end = data_end + (a.plan->pad ? 32u : 0u);
    if (lo >= end) return;
    // The tile's first record: the first whose tail lies behind lo (the tails only grow).  A 64-ary
    // search, every wave on its own: each step the lanes probe 64 evenly spaced tails of the range at
    // once, so the dependent loads are log64 of the batch (three for 46 k records) and not log2.
    const uint32_t lane = threadIdx.x & (kWave - 1);
    uint64_t first = 0;
    for (uint64_t hi = appended; first < hi;) {
        const uint64_t step = (hi - first + kWave - 1) / kWave, probe = first + (lane + 1) * step - 1;
        const uint64_t behind = __ballot(probe >= hi || a.tails[probe] > lo);
        if (behind == 0) {  // the last probe is the range's last tail
            first = hi;
            break;
        }
        const uint32_t f = (uint32_t)__builtin_ctzll(behind);
        const uint64_t cap = first + (f + 1) * step - 1;
        first += f * step;
        hi = cap < hi ? cap : hi;
    }
    // records of the tile: at most one per 32 bytes of it
    const uint64_t left = appended - first;
    const uint32_t cnt = (uint32_t)(left < kTaTileRecs ? left : kTaTileRecs);
    for (uint32_t k = threadIdx.x; k <= cnt; k += kTaThreads) {
        const uint64_t j = first + k;
        tail[k] = (uint32_t)(j == 0 ? a.start : a.tails[j - 1]);
        if (!kIdx) {
            src[k] = a.rec_off[j];  // j <= appended <= n
        } else if (j < appended) {
            const uint64_t s = ta_src<kIdx>(idx, j), at = a.rec_off[s];
            src[k] = at;
            slen[k] = (uint32_t)(a.rec_off[s + 1] - at);
        }
    }
    __syncthreads();
    const uint32_t maxp = a.mtu - 32u;
    const uint32_t w1 = (uint32_t)a.hdr.version | 1u << 16;  // version, flags (byte 1), type 1
    for (uint32_t c = threadIdx.x; c < kTaTile / 16; c += kTaThreads) {
        const uint64_t p = t0 + 16ull * c;
        if (p < a.start || p >= end) continue;
        u32x4 x;
        x.x = x.y = x.z = x.w = 0u;
        if (p >= data_end) {  // the padding frame's header
            if (p == data_end) {
                x.x = (uint32_t)(a.block_bytes - data_end);
                x.y = (uint32_t)a.hdr.version | 0xC0u << 8;
                x.z = (uint32_t)a.hdr.term_offset_base + (uint32_t)data_end;
                x.w = (uint32_t)a.hdr.session_id;
            } else {
                x.x = (uint32_t)a.hdr.stream_id, x.y = (uint32_t)a.hdr.term_id;
            }
        } else {
            // the chunk's record: the first k with tail[k + 1] > p
            uint32_t k = 0;
            for (uint32_t hi = cnt; k < hi;) {
                const uint32_t mid = (k + hi) >> 1;
                if (tail[mid + 1] > (uint32_t)p) hi = mid;
                else k = mid + 1;
            }
            const uint32_t begin = tail[k], q = (uint32_t)p - begin;
            const uint64_t s0 = src[k];
            const uint32_t L = kIdx ? slen[k] : (uint32_t)(src[k + 1] - s0);  // an appended record: at most max_message_length <= 2^30
            uint32_t f = 0, r = q, plen = L, flags = 0xC0u;
            if (L > maxp) {
                f = q / a.mtu;
                r = q - f * a.mtu;
                const uint32_t nfull = L / maxp, rem = L - nfull * maxp;
                plen = f < nfull ? maxp : rem;
                flags = (f == 0 ? 0x80u : 0u) | (f + 1 == nfull + (rem ? 1u : 0u) ? 0x40u : 0u);
            }
            if (r == 0) {
                x.x = 32u + plen;
                x.y = w1 | flags << 8;
                x.z = (uint32_t)a.hdr.term_offset_base + begin + f * a.mtu;
                x.w = (uint32_t)a.hdr.session_id;
            } else if (r == 16) {
                x.x = (uint32_t)a.hdr.stream_id, x.y = (uint32_t)a.hdr.term_id;
            } else if (r - 32u < plen) {  // else: the alignment zeros
                const uint32_t j = r - 32u;
                x = ta_payload(a, s0 + (uint64_t)f * maxp + j, plen - j < 16u ? plen - j : 16u);
            }
        }
        __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(a.block + p));
    }
}
__global__ __launch_bounds__(kTaThreads) void ta_write(TaArgs a, uint32_t tile0) { ta_write_tile<false>(a, TaIdx{}, tile0); }

// sbe_term_append_counted.  a.n is the capacity the plan grids and the block tables were laid out by;
// every launch takes its count from *n_dev.  A plan block past the count leaves its sums empty for
// the scan (which runs over the blocks of the capacity, ta_scan_blocks as it is) and exits; the
// block that holds record n (the one behind the last) still runs the tails.
struct TaCount {
    const uint64_t* n_dev;
    TaIdx idx;
};
__global__ __launch_bounds__(kTaBlk) void ta_sums_counted(TaArgs a, TaCount c) {
    a.n = counted_n(c.n_dev, a.n);
    if (c.idx.at && blockIdx.x == 0 && threadIdx.x == 0) a.counts[2] = 0;  // ta_tails_counted adds the payload bytes up
    if ((uint64_t)blockIdx.x * kTaBlk >= a.n) {
        if (threadIdx.x == 0) {
            a.bsum[blockIdx.x] = 0;
            a.bmin[blockIdx.x] = kTaNone;
        }
        return;
    }
    ta_sums_block<true>(a, c.idx);
}
__global__ __launch_bounds__(kTaBlk) void ta_tails_counted(TaArgs a, TaCount c) {
    a.n = counted_n(c.n_dev, a.n);
    if ((uint64_t)blockIdx.x * kTaBlk > a.n) return;
    ta_tails_block<true>(a, c.idx);
}
__global__ __launch_bounds__(kTaThreads) void ta_write_counted(TaArgs a, TaCount c, uint32_t tile0) {
    ta_write_tile<true>(a, c.idx, tile0);  // the plan holds what the count left: n is not read
}

// counts of a call without records
__global__ void ta_counts_only(uint64_t* counts, uint64_t next) {
    counts[0] = 0;
    counts[1] = next;
    counts[2] = 0;
    counts[3] = SBE_TERM_APPEND_END;
}
