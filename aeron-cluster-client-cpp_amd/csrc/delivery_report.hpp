// delivery_report.hpp — included by sbe_codec.hip inside its anonymous namespace, after delivery_keys.hpp.
//
// The read side of delivery tracking: the three reports examples/pubsub_reconnect_test.cpp prints
// from the sets its callback keeps.
//   sbe_inflight_list_keys   printMessageComparison (:130-204) / printClientOrderAudit (:206-274):
//       the ids of one table that are (not) in another, the first `limit` in std::string order,
//       and the ids of duplicate_delivery_counts (:83-90) as the entries whose value is >= 2
//   sbe_latency_append       the latency the callback records once per client_order_id (:669-691),
//       kept in a log on the device instead of a map
//   sbe_latency_report       printLatencyReport (:276-353): count, sum, min, max, the percentiles
//       by the example's own rank formula, and the rows in ascending (latency, position) order
//
// list_keys, two launches.
//   dr_list_scan    a fixed grid strides over the slots as inf_rehash_kernel does.  A lane reads
//       the word and the value, and the key only of an entry that passes them; the membership
//       probe of `other` is match's read-only walk.  Each workgroup keeps its `limit` smallest
//       candidates sorted in LDS (48 B each: the key as five big-endian words, so that memcmp order
//       is integer order, the length and the slot index).  A round of the stride loop merges the
//       candidates of its lanes in by rank: every element counts the elements below it, and the
//       ranks under `limit` are the next list.  Once the list is full only keys below its last
//       element are candidates, so most rounds merge nothing.
//   dr_list_merge   one workgroup merges the per-workgroup lists the same way, sums the
//       per-workgroup pass counts and writes the rows.
//   The order is total (distinct keys; the slot index breaks a tie a damaged table could hold), so
//   the rows do not depend on where colliding keys sit.
//
// Latency log: 64-B header {u64 capacity, u64 count, u64 dropped, u32 magic}, int64 lat[capacity],
// u64 tag[capacity].  append, three launches: per-workgroup counts of SBE_SENT_FIRST records, one
// workgroup scans them and moves the header's cursor, and every record places itself at cursor +
// (its rank in the call): no atomics on the cursor, so the log is a function of the call sequence.
//
// report: an 8-pass, 8-bit LSD radix sort of (lat ^ 2^63, position) pairs between two workspace
// buffers; pass 0 reads the log itself.  A pass is three launches over tiles of 2048 samples: a
// 256-bin histogram per tile, one exclusive scan over the (digit, tile) matrix, and a scatter that
// ranks a tile in rounds of 256 samples in index order (equal digits of a wave by ballots, the
// waves of a round and the rounds of a tile by running counts), which keeps the sort stable.  One
// last launch sums, copies `sorted` / `order` and reads min, max and the percentile entries.

constexpr uint32_t kDrBlk = 256;
constexpr uint32_t kDrListBlocks = 1024;

struct DrCand {
    uint64_t k[5];  // the key's bytes as big-endian words
    uint32_t len, slot;
};
static_assert(sizeof(DrCand) == 48, "candidate layout");

struct DrTopK {
    DrCand top[2][SBE_LIST_MAX];  // the sorted list, and the one the running merge writes
    DrCand stage[kDrBlk];         // this round's candidates, one per lane
    uint8_t flag[kDrBlk];
};

__device__ __forceinline__ bool dr_less(const DrCand& a, const DrCand& b) {
#pragma unroll
    for (int j = 0; j < 5; ++j)
        if (a.k[j] != b.k[j]) return a.k[j] < b.k[j];
    if (a.len != b.len) return a.len < b.len;
    return a.slot < b.slot;
}

// The `K` smallest of the list (s.top[cur][0, ntop), sorted) and this round's candidates become
// s.top[cur ^ 1]; every thread of the workgroup calls it with the same cur / ntop / K.
__device__ __forceinline__ void dr_merge(DrTopK& s, uint32_t& cur, uint32_t& ntop, uint32_t K, bool have, const DrCand& c) {
    const uint32_t t = threadIdx.x;
    s.flag[t] = have;
    if (have) s.stage[t] = c;
    __syncthreads();
    const DrCand* top = s.top[cur];
    DrCand* next = s.top[cur ^ 1];
    if (have) {
        uint32_t r = 0;
        for (uint32_t j = 0; j < ntop; ++j) r += dr_less(top[j], c);
        for (uint32_t j = 0; j < kDrBlk; ++j)
            if (s.flag[j]) r += dr_less(s.stage[j], c);
        if (r < K) next[r] = c;
    }
    if (t < ntop) {
        const DrCand e = top[t];
        uint32_t r = t;
        for (uint32_t j = 0; j < kDrBlk; ++j)
            if (s.flag[j]) r += dr_less(s.stage[j], e);
        if (r < K) next[r] = e;
    }
    const uint32_t added = (uint32_t)__syncthreads_count(have);
    ntop = ntop + added < K ? ntop + added : K;
    cur ^= 1;
}

struct DrListArgs {
    const uint8_t* table;
    const uint8_t* other;  // or null
    uint32_t flags;
    uint64_t min_value;
    uint32_t limit;
    DrCand* wg_list;    // [workgroups][limit]
    uint32_t* wg_n;     // [workgroups] candidates kept
    uint64_t* wg_pass;  // [workgroups] entries that passed
    uint32_t workgroups;
    uint64_t* count;
    uint8_t* key;
    uint32_t* len;
    uint64_t* value;
    uint8_t* answered;
};

// is k live in the table at `other` (valid header: ocap, otb)?
__device__ __forceinline__ bool dr_member(const uint8_t* other, uint64_t ocap, uint32_t otb, const InfKey& k) {
    const uint64_t h = inf_hash(k);
    const uint32_t tag = inf_tag(h, otb);
    const InfSlot* slots = reinterpret_cast<const InfSlot*>(other + 64);
    uint64_t s = h & (ocap - 1);
    for (uint64_t probe = 0; probe < ocap; ++probe, s = (s + 1) & (ocap - 1)) {
        const InfSlot* sl = slots + s;
        const uint64_t w = sl->word;
        const uint64_t state = w >> 62;
        if (state == kInfEmpty) return false;
        if (state == kInfLive && inf_word_tag(w) == tag && inf_slot_eq(sl, k)) return true;
    }
    return false;
}

__global__ __launch_bounds__(kDrBlk) void dr_list_scan(DrListArgs a) {
    __shared__ DrTopK s;
    const uint32_t t = threadIdx.x, K = a.limit;
    uint64_t cap, ocap = 0;
    uint32_t tb, otb = 0;
    if (!inf_table(a.table, cap, tb)) cap = 0;
    const bool other_ok = a.other && inf_table(a.other, ocap, otb);
    const InfSlot* slots = reinterpret_cast<const InfSlot*>(a.table + 64);
    uint64_t passed = 0;
    uint32_t cur = 0, ntop = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * kDrBlk; base < cap; base += (uint64_t)gridDim.x * kDrBlk) {
        const uint64_t q = base + t;
        bool pass = false;
        DrCand c;
        if (q < cap) {
            const InfSlot* f = slots + q;
            const uint64_t w = f->word;
            if ((w >> 62) == kInfLive) {
                const bool ans = (w & kInfAnswered) != 0;
                pass = f->ts >= a.min_value && !((a.flags & SBE_LIST_ANSWERED) && !ans) &&
                       !((a.flags & SBE_LIST_UNANSWERED) && ans);
                if (pass) {
                    InfKey k;
#pragma unroll
                    for (int j = 0; j < 5; ++j) k.w[j] = f->key[j];
                    k.len = f->len;
                    if (a.other) {
                        const bool member = other_ok && dr_member(a.other, ocap, otb, k);
                        pass = (a.flags & SBE_LIST_IN_OTHER) ? member : !member;
                    }
#pragma unroll
                    for (int j = 0; j < 5; ++j) c.k[j] = __builtin_bswap64(k.w[j]);
                    c.len = k.len;
                    c.slot = (uint32_t)q;
                }
            }
        }
        passed += (uint64_t)__syncthreads_count(pass);
        const bool have = pass && K && (ntop < K || dr_less(c, s.top[cur][K - 1]));
        if (!__syncthreads_or(have)) continue;
        dr_merge(s, cur, ntop, K, have, c);
    }
    if (t < ntop) a.wg_list[(uint64_t)blockIdx.x * K + t] = s.top[cur][t];
    if (t == 0) {
        a.wg_n[blockIdx.x] = ntop;
        a.wg_pass[blockIdx.x] = passed;
    }
}

__global__ __launch_bounds__(kDrBlk) void dr_list_merge(DrListArgs a) {
    __shared__ DrTopK s;
    __shared__ unsigned long long total;
    const uint32_t t = threadIdx.x, K = a.limit;
    if (t == 0) total = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (uint32_t g = t; g < a.workgroups; g += kDrBlk) mine += a.wg_pass[g];
    if (mine) atomicAdd(&total, mine);
    uint32_t cur = 0, ntop = 0;
    const uint64_t all = (uint64_t)a.workgroups * K;
    for (uint64_t base = 0; base < all; base += kDrBlk) {
        const uint64_t idx = base + t;
        bool have = false;
        DrCand c;
        if (idx < all && (uint32_t)(idx % K) < a.wg_n[idx / K]) {
            c = a.wg_list[idx];
            have = ntop < K || dr_less(c, s.top[cur][K - 1]);
        }
        if (!__syncthreads_or(have)) continue;
        dr_merge(s, cur, ntop, K, have, c);
    }
    __syncthreads();
    if (t == 0) a.count[0] = total;
    if (t < ntop) {  // a candidate exists only in a table with a valid header
        const DrCand e = s.top[cur][t];
        const InfSlot* sl = reinterpret_cast<const InfSlot*>(a.table + 64) + e.slot;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const uint64_t w = __builtin_bswap64(e.k[j]);
            __builtin_memcpy(a.key + (uint64_t)t * SBE_INFLIGHT_KEY_MAX + 8 * j, &w, 8);
        }
        a.len[t] = e.len;
        a.value[t] = sl->ts;
        a.answered[t] = (uint8_t)(sl->word & kInfAnswered);
    }
}

// ---- the latency log ----

constexpr uint32_t kLatMagic = 0x4C54414Cu;  // "LATL"
constexpr uint32_t kDrPer = 8;               // records of a thread
constexpr uint32_t kDrTile = kDrBlk * kDrPer;

struct LatHeader {
    uint64_t capacity, count, dropped;
    uint32_t magic, pad;
    uint64_t reserved[4];
};
static_assert(sizeof(LatHeader) == 64, "log layout");

__host__ __device__ inline bool lat_capacity_ok(uint64_t c) { return c >= 1 && c <= (1ull << 31); }

// capacity and count of a log with a valid header
__device__ __forceinline__ bool lat_log(const uint8_t* log, uint64_t& cap, uint64_t& count) {
    const LatHeader* h = reinterpret_cast<const LatHeader*>(log);
    cap = h->capacity;
    count = h->count;
    return h->magic == kLatMagic && lat_capacity_ok(cap) && count <= cap;
}

__global__ __launch_bounds__(kWave) void lat_init_header(uint8_t* log, uint64_t capacity) {
    if (threadIdx.x < 8) reinterpret_cast<uint64_t*>(log)[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        LatHeader* h = reinterpret_cast<LatHeader*>(log);
        h->capacity = capacity;
        h->magic = kLatMagic;
    }
}

// exclusive prefix of v over the workgroup's threads; total: the sum.  sh: kDrBlk words of LDS
__device__ __forceinline__ uint32_t dr_block_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < kDrBlk; off <<= 1) {
        const uint32_t x = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    total = sh[kDrBlk - 1];
    const uint32_t incl = sh[t];
    __syncthreads();
    return incl - v;
}

struct LatAppendArgs {
    uint8_t* log;
    const uint8_t* code;
    const uint64_t* value;
    uint64_t n, now_ns, unit_ns, tag_base;
    uint64_t* cursor;  // workspace: {count before the call, capacity; 0 0 for a log that takes nothing}
    uint32_t* blk;     // workspace: [workgroups] FIRST records, then their exclusive prefix
    uint32_t workgroups;
};

__global__ __launch_bounds__(kDrBlk) void lat_append_count(LatAppendArgs a) {
    const uint64_t i0 = ((uint64_t)blockIdx.x * kDrBlk + threadIdx.x) * kDrPer;
    int mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kDrPer; ++k) mine += i0 + k < a.n && a.code[i0 + k] == SBE_SENT_FIRST;
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) a.blk[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(kDrBlk) void lat_append_scan(LatAppendArgs a) {
    __shared__ uint32_t sh[kDrBlk];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < a.workgroups; base += kDrBlk) {
        const uint32_t g = base + threadIdx.x;
        const uint32_t v = g < a.workgroups ? a.blk[g] : 0;
        uint32_t total;
        const uint32_t ex = dr_block_scan(v, sh, total);
        if (g < a.workgroups) a.blk[g] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        uint64_t cap, count;
        if (lat_log(a.log, cap, count)) {
            LatHeader* h = reinterpret_cast<LatHeader*>(a.log);
            const uint64_t room = cap - count;
            const uint64_t take = carry < room ? carry : room;
            a.cursor[0] = count;
            a.cursor[1] = cap;
            h->count = count + take;
            h->dropped += carry - take;
        } else {
            a.cursor[0] = a.cursor[1] = 0;
        }
    }
}

__global__ __launch_bounds__(kDrBlk) void lat_append_place(LatAppendArgs a) {
    __shared__ uint32_t sh[kDrBlk];
    const uint64_t i0 = ((uint64_t)blockIdx.x * kDrBlk + threadIdx.x) * kDrPer;
    uint32_t first = 0, mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kDrPer; ++k)
        if (i0 + k < a.n && a.code[i0 + k] == SBE_SENT_FIRST) {
            first |= 1u << k;
            ++mine;
        }
    uint32_t total;
    const uint32_t ex = dr_block_scan(mine, sh, total);
    const uint64_t cap = a.cursor[1];
    uint64_t at = a.cursor[0] + a.blk[blockIdx.x] + ex;
    int64_t* lat = reinterpret_cast<int64_t*>(a.log + 64);
    uint64_t* tag = reinterpret_cast<uint64_t*>(a.log + 64) + cap;
#pragma unroll
    for (uint32_t k = 0; k < kDrPer; ++k) {
        if (!(first >> k & 1)) continue;
        if (at < cap) {
            lat[at] = (int64_t)(a.now_ns - a.value[i0 + k]) / (int64_t)a.unit_ns;
            tag[at] = a.tag_base + (i0 + k);
        }
        ++at;
    }
}

// ---- the report: a stable LSD radix sort of (lat, position) ----

constexpr uint32_t kDrSortBlocks = 1024;
constexpr uint64_t kDrSign = 1ull << 63;
constexpr uint32_t kDrScanPer = 16;  // matrix entries of a thread per round of the scan

struct LatSortArgs {
    const uint8_t* log;
    uint64_t ws_cap;  // samples the workspace holds
    uint64_t* key[2];
    uint32_t* idx[2];
    uint32_t* hist;  // [256][tiles]
};

// samples to sort: 0 for a log without a valid header or one the workspace cannot hold
__device__ __forceinline__ uint64_t lat_sort_count(const LatSortArgs& a) {
    uint64_t cap, count;
    return lat_log(a.log, cap, count) && count <= a.ws_cap ? count : 0;
}
// pass p reads the log (0), buffer 0 (odd p) or 1, and writes buffer p & 1: pass 7 leaves buffer 1
__device__ __forceinline__ uint64_t lat_sort_key(const LatSortArgs& a, uint32_t p, uint64_t i) {
    return p == 0 ? reinterpret_cast<const uint64_t*>(a.log + 64)[i] ^ kDrSign : a.key[(p & 1) ^ 1][i];
}

__global__ __launch_bounds__(kDrBlk) void lat_sort_hist(LatSortArgs a, uint32_t p) {
    __shared__ uint32_t h[256];
    const uint32_t t = threadIdx.x;
    const uint64_t n = lat_sort_count(a), tiles = (n + kDrTile - 1) / kDrTile;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        h[t] = 0;
        __syncthreads();
        for (uint32_t r = 0; r < kDrPer; ++r) {
            const uint64_t i = tile * kDrTile + r * kDrBlk + t;
            if (i < n) atomicAdd(&h[(uint32_t)(lat_sort_key(a, p, i) >> (8 * p)) & 255u], 1u);
        }
        __syncthreads();
        a.hist[(uint64_t)t * tiles + tile] = h[t];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kDrBlk) void lat_sort_scan(LatSortArgs a) {
    __shared__ uint32_t sh[kDrBlk];
    const uint64_t n = lat_sort_count(a), tiles = (n + kDrTile - 1) / kDrTile, all = 256 * tiles;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < all; base += (uint64_t)kDrBlk * kDrScanPer) {
        const uint64_t i0 = base + (uint64_t)threadIdx.x * kDrScanPer;
        uint32_t v[kDrScanPer], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kDrScanPer; ++k) {
            v[k] = i0 + k < all ? a.hist[i0 + k] : 0;
            sum += v[k];
        }
        uint32_t total;
        uint32_t run = carry + dr_block_scan(sum, sh, total);
#pragma unroll
        for (uint32_t k = 0; k < kDrScanPer; ++k) {
            if (i0 + k < all) a.hist[i0 + k] = run;
            run += v[k];
        }
        carry += total;
    }
}

__global__ __launch_bounds__(kDrBlk) void lat_sort_scatter(LatSortArgs a, uint32_t p) {
    __shared__ uint32_t run[256];    // where the next sample of a digit goes
    __shared__ uint32_t wc[4][256];  // samples of a digit in each wave of the round
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const uint64_t n = lat_sort_count(a), tiles = (n + kDrTile - 1) / kDrTile;
    uint64_t* dk = a.key[p & 1];
    uint32_t* di = a.idx[p & 1];
    const uint32_t* si = a.idx[(p & 1) ^ 1];
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        run[t] = a.hist[(uint64_t)t * tiles + tile];
#pragma unroll
        for (int w = 0; w < 4; ++w) wc[w][t] = 0;
        __syncthreads();
        for (uint32_t r = 0; r < kDrPer; ++r) {
            const uint64_t i = tile * kDrTile + r * kDrBlk + t;
            const bool valid = i < n;
            const uint64_t key = valid ? lat_sort_key(a, p, i) : 0;
            const uint32_t pos = valid ? (p == 0 ? (uint32_t)i : si[i]) : 0;
            const uint32_t d = (uint32_t)(key >> (8 * p)) & 255u;
            uint64_t peers = __ballot(valid);  // the lanes of this wave with the same digit
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1u;
                const uint64_t m = __ballot(valid && bit);
                peers &= bit ? m : ~m;
            }
            const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
            if (valid && rank == 0) wc[wave][d] = (uint32_t)__popcll(peers);
            __syncthreads();
            if (valid) {
                uint32_t at = run[d] + rank;
                for (uint32_t w = 0; w < wave; ++w) at += wc[w][d];
                dk[at] = key;
                di[at] = pos;
            }
            __syncthreads();
            run[t] += wc[0][t] + wc[1][t] + wc[2][t] + wc[3][t];
#pragma unroll
            for (int w = 0; w < 4; ++w) wc[w][t] = 0;
            __syncthreads();
        }
    }
}

struct LatReportArgs {
    LatSortArgs s;
    double pct[SBE_LAT_MAX_PCT];
    uint32_t n_pct;
    uint64_t* count;
    int64_t* stats;  // zeroed before the launch
    int64_t* pct_value;
    uint64_t* pct_index;
    int64_t* sorted;  // or null
    uint32_t* order;  // or null
};

__global__ __launch_bounds__(kDrBlk) void lat_report_final(LatReportArgs a) {
    const uint64_t n = lat_sort_count(a.s);
    const uint64_t* key = a.s.key[1];
    const uint32_t* idx = a.s.idx[1];
    uint64_t sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kDrBlk + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kDrBlk) {
        const uint64_t v = key[i] ^ kDrSign;
        sum += v;
        if (a.sorted) a.sorted[i] = (int64_t)v;
        if (a.order) a.order[i] = idx[i];
    }
    __shared__ unsigned long long total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    if (sum) atomicAdd(&total, (unsigned long long)sum);
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(reinterpret_cast<unsigned long long*>(a.stats), total);
    if (blockIdx.x != 0) return;
    if (threadIdx.x == 0) {
        a.count[0] = n;
        a.stats[1] = n ? (int64_t)(key[0] ^ kDrSign) : 0;
        a.stats[2] = n ? (int64_t)(key[n - 1] ^ kDrSign) : 0;
    }
    if (threadIdx.x < a.n_pct) {
        uint64_t at = 0;
        int64_t v = 0;
        if (n) {  // printLatencyReport's rank, :322-326, in its order of operations
            const double rank = (a.pct[threadIdx.x] / 100.0) * (double)n;
            at = rank <= 0.0 ? 0 : (uint64_t)ceil(rank) - 1;
            at = at < n - 1 ? at : n - 1;
            v = (int64_t)(key[at] ^ kDrSign);
        }
        a.pct_value[threadIdx.x] = v;
        a.pct_index[threadIdx.x] = at;
    }
}
