// inflight.hpp — included by sbe_codec.hip inside its anonymous namespace, after order_publish.hpp.
//
// Ack correlation on the device: ClusterClient::remember_outgoing (src/cluster_client.cpp:1920-1922,
// the emplace into inflight_, include/aeron_cluster/cluster_client.hpp:420) and on_ack_default
// (:1924-1941, find / erase) for whole batches, on a hash table that lives in caller-owned device
// memory across calls (sbe_inflight_*).
//
// Table: one 64-B header, then `capacity` (a power of two) slots of 64 B, linear probing from a
// 64-bit hash of the zero-padded key and its length.
//   slot  +0  u64 word   state << 62 | tag << 32 | record index (while PENDING) or the answered
//                        bit (bit 0, while LIVE: a lookup_keys call has reported the entry's value)
//         +8  u64 ts     the value: a send time (remember) or a number of deliveries (note_keys)
//         +16 40 key bytes, zero-padded
//         +56 u32 claim  smallest ack index of the running match call, 0xFFFFFFFF otherwise
//         +60 u32 len
// States: EMPTY -> PENDING -> LIVE -> ERASED.  A slot never returns to EMPTY (inserts do not reuse
// erased slots; sbe_inflight_rehash reclaims them), so "the first slot of the chain that is empty
// or holds this key" is the same slot for every record of a key, whenever it walks.
//
// Every per-record call is two launches, one lane per record.
//   remember, launch A   walk the chain.  EMPTY: 64-bit CAS to PENDING(tag, i).  PENDING with an
//       equal tag: compare with the owner's key, read from the input arena; equal: atomicMin on the
//       word hands the slot to the smaller index.  LIVE with an equal tag: compare with the stored
//       bytes (an earlier call wrote them).  Within the launch a slot only goes from EMPTY to
//       PENDING for one fixed key, so all records of a key end on one slot; its index goes to the
//       workspace.
//   remember, launch B   the record whose index the word still holds writes key, ts, len, claim
//       and the LIVE word: INSERTED.  Every other record on that slot is DUPLICATE.
//   match, launch A      find the LIVE slot of the id (EMPTY ends the chain), atomicMin(claim, i).
//   match, launch B      the record whose index the claim holds is MATCHED: it reads ts and stores
//       the ERASED word.  The others are UNMATCHED.
//   note, launch A       remember's walk with keys anywhere in a buffer; every record that ends on
//       a slot adds 1 to its value (an EMPTY slot's value is 0: init's memset, and no slot is reused).
//   note, launch B       the owner of a PENDING slot writes key, len, claim and the LIVE word, not
//       the value: NEW.  The others are AGAIN.  All read the finished sum.
//   lookup, launch A     match's walk; atomicMin(claim, i) unless the entry is answered; the
//       workspace word is the slot index with "was answered when found" in bit 31, and code[i]
//       already holds the outcome of every record that found no entry.
//   lookup, launch B     the record whose index the claim holds is FIRST: it reads the value, sets
//       the answered bit and gives the claim back.  The others are REPEAT.
// Within a launch no lane reads bytes another lane of that launch writes, except the state and
// claim words, and those go through device-scope atomics: no fences or flags.  Which of two
// colliding keys gets the earlier slot depends on timing; what a call reports does not.
//
// The header is device memory, so the host cannot look at it without a copy: the kernels check it
// (magic, capacity) and treat a table without a valid header as holding nothing and having no room.

constexpr uint32_t kInfMagic = 0x544C4649u;  // "IFLT"
constexpr uint32_t kInfBlk = 256;
constexpr uint64_t kInfEmpty = 0, kInfPending = 1, kInfLive = 2, kInfErased = 3;
constexpr uint32_t kInfNoClaim = 0xFFFFFFFFu;
// workspace entries: a slot index (< 2^31) or one of these
constexpr uint32_t kInfWsSkipped = 0xFFFFFFF0u, kInfWsTooLong = 0xFFFFFFF1u, kInfWsFull = 0xFFFFFFF2u,
                   kInfWsNone = 0xFFFFFFF3u, kInfWsUnmatched = 0xFFFFFFF4u, kInfWsLong = 0xFFFFFFF5u;

struct InfHeader {
    uint64_t capacity, live, used;
    uint32_t tag_bits, magic;
    uint64_t answered;  // live entries whose answered bit is set
    uint64_t reserved[3];
};
struct InfSlot {
    uint64_t word, ts, key[5];
    uint32_t claim, len;
};
static_assert(sizeof(InfHeader) == 64 && sizeof(InfSlot) == 64, "table layout");
static_assert(SBE_INFLIGHT_KEY_MAX == 40, "five key words");

struct InfKey {
    uint64_t w[5];
    uint32_t len;
};

__host__ __device__ inline bool inf_capacity_ok(uint64_t c) { return c >= 64 && c <= (1ull << 31) && (c & (c - 1)) == 0; }

__device__ __forceinline__ uint64_t inf_word(uint64_t state, uint32_t tag, uint32_t idx) {
    return state << 62 | (uint64_t)tag << 32 | idx;
}
__device__ __forceinline__ uint32_t inf_word_tag(uint64_t w) { return (uint32_t)(w >> 32) & 0x3fffffffu; }
constexpr uint64_t kInfAnswered = 1;  // bit 0 of a LIVE word

// key bytes p[0, len), len <= 40, zero-padded into five words; reads no byte past p + len
__device__ __forceinline__ void inf_load_key(const uint8_t* p, uint32_t len, InfKey& k) {
    k.len = len;
#pragma unroll
    for (uint32_t j = 0; j < 5; ++j) {
        uint64_t v = 0;
        if (len >= 8 * j + 8) {
            __builtin_memcpy(&v, p + 8 * j, 8);
        } else if (len > 8 * j) {
            for (uint32_t t = 0; t < len - 8 * j; ++t) v |= (uint64_t)p[8 * j + t] << (8 * t);
        }
        k.w[j] = v;
    }
}
__device__ __forceinline__ uint64_t inf_hash(const InfKey& k) {
    uint64_t h = (k.len + 1) * 0xD6E8FEB86659FD93ull;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        h = (h ^ k.w[j]) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
    }
    h *= 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 32);
}
__device__ __forceinline__ uint32_t inf_tag(uint64_t h, uint32_t tag_bits) { return (uint32_t)(h >> 34) & ((1u << tag_bits) - 1u); }

__device__ __forceinline__ bool inf_key_eq(const InfKey& a, const InfKey& b) {
    return a.len == b.len && a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3] &&
           a.w[4] == b.w[4];
}
__device__ __forceinline__ bool inf_slot_eq(const InfSlot* s, const InfKey& k) {
    return s->len == k.len && s->key[0] == k.w[0] && s->key[1] == k.w[1] && s->key[2] == k.w[2] && s->key[3] == k.w[3] &&
           s->key[4] == k.w[4];
}

// capacity and tag bits of a table with a valid header
__device__ __forceinline__ bool inf_table(const uint8_t* table, uint64_t& cap, uint32_t& tag_bits) {
    const InfHeader* h = reinterpret_cast<const InfHeader*>(table);
    cap = h->capacity;
    tag_bits = h->tag_bits;
    return h->magic == kInfMagic && inf_capacity_ok(cap) && tag_bits >= 1 && tag_bits <= 30;
}
__device__ __forceinline__ uint64_t inf_ld(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Launch A of an inserting call (remember, note): the slot of key k for record i, or kInfWsFull.
// The first slot of the chain that is EMPTY (taken by CAS as PENDING(tag, i)), PENDING for an equal
// key (atomicMin hands it to the smaller index) or LIVE with an equal key.  owner_key(j, o) loads
// the key of record j of the running call into o; false: j is not a record that can own a slot.
template <class OwnerKey>
__device__ __forceinline__ uint32_t inf_claim_slot(uint8_t* table, uint64_t cap, uint64_t h, uint32_t tag, uint32_t i,
                                                   const InfKey& k, const OwnerKey& owner_key) {
    InfSlot* slots = reinterpret_cast<InfSlot*>(table + 64);
    uint64_t s = h & (cap - 1);
    for (uint64_t probe = 0; probe < cap; ++probe, s = (s + 1) & (cap - 1)) {
        InfSlot* sl = slots + s;
        uint64_t w = inf_ld(&sl->word);
        if ((w >> 62) == kInfEmpty) {
            unsigned long long seen = 0;
            if (__hip_atomic_compare_exchange_strong(reinterpret_cast<unsigned long long*>(&sl->word), &seen,
                                                     (unsigned long long)inf_word(kInfPending, tag, i), __ATOMIC_RELAXED,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                return (uint32_t)s;
            w = seen;  // another record took it first: look at what it holds
        }
        const uint64_t state = w >> 62;
        if (state == kInfErased || inf_word_tag(w) != tag) continue;
        if (state == kInfPending) {
            InfKey o;
            if (!owner_key((uint32_t)w, o) || !inf_key_eq(o, k)) continue;
            __hip_atomic_fetch_min(reinterpret_cast<unsigned long long*>(&sl->word),
                                   (unsigned long long)inf_word(kInfPending, tag, i), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            return (uint32_t)s;
        }
        if (inf_slot_eq(sl, k)) return (uint32_t)s;  // LIVE
    }
    return kInfWsFull;
}

__global__ __launch_bounds__(kWave) void inf_init_header(uint8_t* table, uint64_t capacity, uint32_t tag_bits) {
    if (threadIdx.x == 0) {
        InfHeader* h = reinterpret_cast<InfHeader*>(table);
        h->capacity = capacity;
        h->live = h->used = 0;
        h->tag_bits = tag_bits;
        h->magic = kInfMagic;
    }
}

struct InfRemArgs {
    uint8_t* table;
    const uint8_t* arena;
    const uint32_t* key_off;
    const uint32_t* key_len;
    uint32_t stride;
    const uint64_t* ts;
    uint64_t ts_default;
    const uint8_t* mask;
    uint64_t n;
    uint8_t* status;
    uint32_t* ws;
};

__global__ __launch_bounds__(kInfBlk) void inf_remember_find(InfRemArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kInfBlk + threadIdx.x;
    if (i >= a.n) return;
    if (a.mask && !a.mask[i]) {
        a.ws[i] = kInfWsSkipped;
        return;
    }
    const uint32_t len = a.key_len[i * a.stride];
    if (len > SBE_INFLIGHT_KEY_MAX) {
        a.ws[i] = kInfWsTooLong;
        return;
    }
    uint64_t cap;
    uint32_t tb;
    if (!inf_table(a.table, cap, tb)) {
        a.ws[i] = kInfWsFull;
        return;
    }
    InfKey k;
    inf_load_key(a.arena + a.key_off[i * a.stride], len, k);
    const uint64_t h = inf_hash(k);
    const uint32_t tag = inf_tag(h, tb);
    a.ws[i] = inf_claim_slot(a.table, cap, h, tag, (uint32_t)i, k, [&](uint64_t j, InfKey& o) {
        const uint32_t jl = a.key_len[j * a.stride];
        if (jl > SBE_INFLIGHT_KEY_MAX) return false;
        inf_load_key(a.arena + a.key_off[j * a.stride], jl, o);
        return true;
    });
}

__global__ __launch_bounds__(kInfBlk) void inf_remember_commit(InfRemArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kInfBlk + threadIdx.x;
    uint32_t st = SBE_INF_SKIPPED;
    bool inserted = false;
    if (i < a.n) {
        const uint32_t c = a.ws[i];
        if (c == kInfWsSkipped) {
            st = SBE_INF_SKIPPED;
        } else if (c == kInfWsTooLong) {
            st = SBE_INF_KEY_TOO_LONG;
        } else if (c == kInfWsFull) {
            st = SBE_INF_FULL;
        } else {
            InfSlot* sl = reinterpret_cast<InfSlot*>(a.table + 64) + c;
            const uint64_t w = inf_ld(&sl->word);
            st = SBE_INF_DUPLICATE;
            if ((w >> 62) == kInfPending && (uint32_t)w == (uint32_t)i) {
                InfKey k;
                inf_load_key(a.arena + a.key_off[i * a.stride], a.key_len[i * a.stride], k);
                const uint64_t t = a.ts ? a.ts[i] : 0;
                sl->ts = t ? t : a.ts_default;
#pragma unroll
                for (int j = 0; j < 5; ++j) sl->key[j] = k.w[j];
                sl->claim = kInfNoClaim;
                sl->len = k.len;
                __hip_atomic_store(&sl->word, inf_word(kInfLive, inf_word_tag(w), 0), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
                st = SBE_INF_INSERTED;
                inserted = true;
            }
        }
        if (a.status) a.status[i] = (uint8_t)st;
    }
    const int cnt = __syncthreads_count(inserted);
    if (threadIdx.x == 0 && cnt) {
        InfHeader* h = reinterpret_cast<InfHeader*>(a.table);
        atomicAdd(reinterpret_cast<unsigned long long*>(&h->live), (unsigned long long)cnt);
        atomicAdd(reinterpret_cast<unsigned long long*>(&h->used), (unsigned long long)cnt);
    }
}

struct InfMatchArgs {
    uint8_t* table;
    const uint8_t* in;
    const uint64_t* rec_off;
    uint64_t n;
    const uint8_t* status;
    const uint64_t* ts;
    const uint32_t* view_off;
    const uint32_t* view_len;
    uint8_t* code;
    uint64_t* base_ns;
    uint64_t* counts;
    uint32_t* ws;
};

__global__ __launch_bounds__(kInfBlk) void inf_match_find(InfMatchArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kInfBlk + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t st = a.status[i];
    if (st != SBE_ST_EG_ACK && st != SBE_ST_EG_ACK_SIMPLE) {
        a.ws[i] = kInfWsNone;
        return;
    }
    uint32_t res = kInfWsUnmatched;
    uint64_t cap;
    uint32_t tb;
    if (st == SBE_ST_EG_ACK) {
        // the id view, kept inside the record whatever the descriptors say
        const uint64_t b = a.rec_off[i], e = a.rec_off[i + 1];
        const uint64_t L64 = e > b ? e - b : 0;
        const uint32_t L = L64 > 0xffffffffull ? 0xffffffffu : (uint32_t)L64;
        uint32_t vo = a.view_off[5 * i], vl = a.view_len[5 * i];
        vo = vo <= L ? vo : L;
        vl = vl <= L - vo ? vl : L - vo;
        if (vl > SBE_INFLIGHT_KEY_MAX) {
            res = kInfWsLong;
        } else if (vl && inf_table(a.table, cap, tb)) {
            InfKey k;
            inf_load_key(a.in + b + vo, vl, k);
            const uint64_t h = inf_hash(k);
            const uint32_t tag = inf_tag(h, tb);
            InfSlot* slots = reinterpret_cast<InfSlot*>(a.table + 64);
            uint64_t s = h & (cap - 1);
            for (uint64_t probe = 0; probe < cap; ++probe, s = (s + 1) & (cap - 1)) {
                InfSlot* sl = slots + s;
                const uint64_t w = sl->word;  // no launch of a match call writes a word another lane reads
                const uint64_t state = w >> 62;
                if (state == kInfEmpty) break;
                if (state != kInfLive || inf_word_tag(w) != tag || !inf_slot_eq(sl, k)) continue;
                __hip_atomic_fetch_min(&sl->claim, (uint32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                res = (uint32_t)s;
                break;
            }
        }
    }
    a.ws[i] = res;
}

__global__ __launch_bounds__(kInfBlk) void inf_match_commit(InfMatchArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kInfBlk + threadIdx.x;
    bool matched = false, missed = false, answered = false;
    if (i < a.n) {
        const uint32_t c = a.ws[i];
        uint32_t code = SBE_ACK_UNMATCHED;
        uint64_t base = 0;
        if (c == kInfWsNone) {
            code = SBE_ACK_NONE;
        } else if (c == kInfWsUnmatched || c == kInfWsLong) {
            code = c == kInfWsLong ? SBE_ACK_LONG_ID : SBE_ACK_UNMATCHED;
            base = a.ts[i];
        } else {
            InfSlot* sl = reinterpret_cast<InfSlot*>(a.table + 64) + c;
            if (sl->claim == (uint32_t)i) {
                code = SBE_ACK_MATCHED;
                base = sl->ts;
                const uint64_t w = sl->word;
                answered = (w & kInfAnswered) != 0;
                sl->word = inf_word(kInfErased, inf_word_tag(w), 0);
            } else {
                base = a.ts[i];
            }
        }
        a.code[i] = (uint8_t)code;
        a.base_ns[i] = base;
        matched = code == SBE_ACK_MATCHED;
        missed = code == SBE_ACK_UNMATCHED || code == SBE_ACK_LONG_ID;
    }
    const int nm = __syncthreads_count(matched);
    const int nu = __syncthreads_count(missed);
    const int na = __syncthreads_count(answered);
    if (threadIdx.x == 0) {
        if (nm) {
            InfHeader* h = reinterpret_cast<InfHeader*>(a.table);
            atomicAdd(reinterpret_cast<unsigned long long*>(&h->live), (unsigned long long)(-(long long)nm));
            if (na) atomicAdd(reinterpret_cast<unsigned long long*>(&h->answered), (unsigned long long)(-(long long)na));
            if (a.counts) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts), (unsigned long long)nm);
        }
        if (nu && a.counts) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts + 1), (unsigned long long)nu);
    }
}

// Every LIVE entry of src into dst (initialised, empty).  The keys of a table are distinct, so an
// insert compares nothing: the first EMPTY slot of the chain, taken by CAS, is the entry's.
constexpr uint32_t kInfRehashBlocks = 2048;
__global__ __launch_bounds__(kInfBlk) void inf_rehash_kernel(const uint8_t* src, uint8_t* dst) {
    uint64_t scap, dcap;
    uint32_t stb, dtb;
    int moved = 0, marked = 0;
    if (inf_table(src, scap, stb) && inf_table(dst, dcap, dtb)) {
        const InfSlot* from = reinterpret_cast<const InfSlot*>(src + 64);
        InfSlot* to = reinterpret_cast<InfSlot*>(dst + 64);
        for (uint64_t q = (uint64_t)blockIdx.x * kInfBlk + threadIdx.x; q < scap; q += (uint64_t)gridDim.x * kInfBlk) {
            const InfSlot* f = from + q;
            const uint64_t fw = f->word;
            if ((fw >> 62) != kInfLive) continue;
            InfKey k;
#pragma unroll
            for (int j = 0; j < 5; ++j) k.w[j] = f->key[j];
            k.len = f->len;
            const uint64_t h = inf_hash(k);
            const unsigned long long live = inf_word(kInfLive, inf_tag(h, dtb), (uint32_t)(fw & kInfAnswered));
            uint64_t s = h & (dcap - 1);
            for (uint64_t probe = 0; probe < dcap; ++probe, s = (s + 1) & (dcap - 1)) {
                InfSlot* t = to + s;
                if ((inf_ld(&t->word) >> 62) != kInfEmpty) continue;
                unsigned long long seen = 0;
                if (!__hip_atomic_compare_exchange_strong(reinterpret_cast<unsigned long long*>(&t->word), &seen, live,
                                                          __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    continue;
                t->ts = f->ts;
#pragma unroll
                for (int j = 0; j < 5; ++j) t->key[j] = k.w[j];
                t->claim = kInfNoClaim;
                t->len = k.len;
                ++moved;
                marked += (int)(fw & kInfAnswered);
                break;
            }
        }
    }
    // per-thread counts summed over the block: one pair of atomics per workgroup
    __shared__ int total, total_marked;
    if (threadIdx.x == 0) total = total_marked = 0;
    __syncthreads();
    if (moved) atomicAdd(&total, moved);
    if (marked) atomicAdd(&total_marked, marked);
    __syncthreads();
    if (threadIdx.x == 0 && total) {
        InfHeader* h = reinterpret_cast<InfHeader*>(dst);
        atomicAdd(reinterpret_cast<unsigned long long*>(&h->live), (unsigned long long)total);
        atomicAdd(reinterpret_cast<unsigned long long*>(&h->used), (unsigned long long)total);
        if (total_marked) atomicAdd(reinterpret_cast<unsigned long long*>(&h->answered), (unsigned long long)total_marked);
    }
}

// ---- keys anywhere in a buffer: note_keys (test-and-insert that counts) and lookup_keys ----

struct InfKeysArgs {
    uint8_t* table;
    const uint8_t* buf;
    uint64_t buf_bytes;
    const uint64_t* key_pos;
    const uint32_t* key_len;
    uint64_t n;
    uint8_t* code;
    uint32_t* count;   // note
    uint64_t* value;   // lookup
    uint64_t* totals;  // or null
    uint32_t* ws;
};

// key i clamped into [0, buf_bytes): no byte at or past buf_bytes is read
__device__ __forceinline__ void inf_key_range(const InfKeysArgs& a, uint64_t i, uint64_t& pos, uint32_t& len) {
    const uint64_t p = a.key_pos[i];
    pos = p <= a.buf_bytes ? p : a.buf_bytes;
    const uint64_t room = a.buf_bytes - pos;
    const uint32_t l = a.key_len[i];
    len = l <= room ? l : (uint32_t)room;
}

__global__ __launch_bounds__(kInfBlk) void inf_note_find(InfKeysArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kInfBlk + threadIdx.x;
    if (i >= a.n) return;
    if (a.key_len[i] == SBE_NO_KEY) {
        a.ws[i] = kInfWsNone;
        return;
    }
    uint64_t pos;
    uint32_t len;
    inf_key_range(a, i, pos, len);
    if (len > SBE_INFLIGHT_KEY_MAX) {
        a.ws[i] = kInfWsTooLong;
        return;
    }
    uint64_t cap;
    uint32_t tb;
    if (!inf_table(a.table, cap, tb)) {
        a.ws[i] = kInfWsFull;
        return;
    }
    InfKey k;
    inf_load_key(a.buf + pos, len, k);
    const uint64_t h = inf_hash(k);
    const uint32_t tag = inf_tag(h, tb);
    const uint32_t res = inf_claim_slot(a.table, cap, h, tag, (uint32_t)i, k, [&](uint64_t j, InfKey& o) {
        if (j >= a.n || a.key_len[j] == SBE_NO_KEY) return false;
        uint64_t jp;
        uint32_t jl;
        inf_key_range(a, j, jp, jl);
        if (jl > SBE_INFLIGHT_KEY_MAX) return false;
        inf_load_key(a.buf + jp, jl, o);
        return true;
    });
    if (res != kInfWsFull)  // one more delivery of this slot's key
        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(&reinterpret_cast<InfSlot*>(a.table + 64)[res].ts), 1ull,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.ws[i] = res;
}

__global__ __launch_bounds__(kInfBlk) void inf_note_commit(InfKeysArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kInfBlk + threadIdx.x;
    bool fresh = false, again = false;
    if (i < a.n) {
        const uint32_t c = a.ws[i];
        uint32_t code = SBE_DLV_NONE, count = 0;
        if (c == kInfWsNone) {
            code = SBE_DLV_NONE;
        } else if (c == kInfWsTooLong) {
            code = SBE_DLV_LONG;
        } else if (c == kInfWsFull) {
            code = SBE_DLV_FULL;
        } else {
            InfSlot* sl = reinterpret_cast<InfSlot*>(a.table + 64) + c;
            const uint64_t w = inf_ld(&sl->word);
            code = SBE_DLV_AGAIN;
            count = (uint32_t)(sl->ts - 1);  // launch A finished every add
            if ((w >> 62) == kInfPending && (uint32_t)w == (uint32_t)i) {
                uint64_t pos;
                uint32_t len;
                inf_key_range(a, i, pos, len);
                InfKey k;
                inf_load_key(a.buf + pos, len, k);
#pragma unroll
                for (int j = 0; j < 5; ++j) sl->key[j] = k.w[j];
                sl->claim = kInfNoClaim;
                sl->len = k.len;
                __hip_atomic_store(&sl->word, inf_word(kInfLive, inf_word_tag(w), 0), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
                code = SBE_DLV_NEW;
            }
        }
        a.code[i] = (uint8_t)code;
        a.count[i] = count;
        fresh = code == SBE_DLV_NEW;
        again = code == SBE_DLV_AGAIN;
    }
    const int nf = __syncthreads_count(fresh);
    const int na = __syncthreads_count(again);
    if (threadIdx.x == 0) {
        if (nf) {
            InfHeader* h = reinterpret_cast<InfHeader*>(a.table);
            atomicAdd(reinterpret_cast<unsigned long long*>(&h->live), (unsigned long long)nf);
            atomicAdd(reinterpret_cast<unsigned long long*>(&h->used), (unsigned long long)nf);
            if (a.totals) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals), (unsigned long long)nf);
        }
        if (na && a.totals) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals + 1), (unsigned long long)na);
    }
}

constexpr uint32_t kInfWsAnswered = 0x80000000u;  // slot indices are below 2^31

__global__ __launch_bounds__(kInfBlk) void inf_lookup_find(InfKeysArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kInfBlk + threadIdx.x;
    if (i >= a.n) return;
    uint32_t code = SBE_SENT_UNKNOWN, res = 0;
    if (a.key_len[i] == SBE_NO_KEY) {
        code = SBE_SENT_NONE;
    } else {
        uint64_t pos, cap;
        uint32_t len, tb;
        inf_key_range(a, i, pos, len);
        if (len > SBE_INFLIGHT_KEY_MAX) {
            code = SBE_SENT_LONG;
        } else if (inf_table(a.table, cap, tb)) {
            InfKey k;
            inf_load_key(a.buf + pos, len, k);
            const uint64_t h = inf_hash(k);
            const uint32_t tag = inf_tag(h, tb);
            InfSlot* slots = reinterpret_cast<InfSlot*>(a.table + 64);
            uint64_t s = h & (cap - 1);
            for (uint64_t probe = 0; probe < cap; ++probe, s = (s + 1) & (cap - 1)) {
                InfSlot* sl = slots + s;
                const uint64_t w = sl->word;  // launch A of a lookup writes no word
                const uint64_t state = w >> 62;
                if (state == kInfEmpty) break;
                if (state != kInfLive || inf_word_tag(w) != tag || !inf_slot_eq(sl, k)) continue;
                code = SBE_SENT_REPEAT;  // launch B decides between FIRST and REPEAT
                res = (uint32_t)s;
                if (w & kInfAnswered)
                    res |= kInfWsAnswered;
                else
                    __hip_atomic_fetch_min(&sl->claim, (uint32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    a.code[i] = (uint8_t)code;
    a.ws[i] = res;
}

__global__ __launch_bounds__(kInfBlk) void inf_lookup_commit(InfKeysArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kInfBlk + threadIdx.x;
    bool first = false, repeat = false, unknown = false;
    if (i < a.n) {
        uint32_t code = a.code[i];
        uint64_t value = 0;
        if (code == SBE_SENT_REPEAT) {
            const uint32_t c = a.ws[i];
            // an entry answered before the call took no claim; otherwise the claim is the smallest
            // index of the call, and only that lane writes the slot
            if (!(c & kInfWsAnswered)) {
                InfSlot* sl = reinterpret_cast<InfSlot*>(a.table + 64) + c;
                if (__hip_atomic_load(&sl->claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)i) {
                    code = SBE_SENT_FIRST;
                    value = sl->ts;
                    sl->word |= kInfAnswered;
                    __hip_atomic_store(&sl->claim, kInfNoClaim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            a.code[i] = (uint8_t)code;
        }
        a.value[i] = value;
        first = code == SBE_SENT_FIRST;
        repeat = code == SBE_SENT_REPEAT;
        unknown = code == SBE_SENT_UNKNOWN || code == SBE_SENT_LONG;
    }
    const int nf = __syncthreads_count(first);
    const int nr = __syncthreads_count(repeat);
    const int nu = __syncthreads_count(unknown);
    if (threadIdx.x == 0) {
        if (nf) atomicAdd(reinterpret_cast<unsigned long long*>(&reinterpret_cast<InfHeader*>(a.table)->answered),
                          (unsigned long long)nf);
        if (a.totals) {
            if (nf) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals), (unsigned long long)nf);
            if (nr) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals + 1), (unsigned long long)nr);
            if (nu) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals + 2), (unsigned long long)nu);
        }
    }
}

// The value of every LIVE slot back to one delivery (clear_duplicate_tracking: the per-id counts of
// record_duplicate_delivery start again, so the next redelivery of a known id reports 1).
__global__ __launch_bounds__(kInfBlk) void inf_reset_values_kernel(uint8_t* table) {
    uint64_t cap;
    uint32_t tb;
    if (!inf_table(table, cap, tb)) return;
    InfSlot* slots = reinterpret_cast<InfSlot*>(table + 64);
    for (uint64_t q = (uint64_t)blockIdx.x * kInfBlk + threadIdx.x; q < cap; q += (uint64_t)gridDim.x * kInfBlk)
        if ((slots[q].word >> 62) == kInfLive) slots[q].ts = 1;
}
