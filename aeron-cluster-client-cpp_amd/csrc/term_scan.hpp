// term_scan.hpp — included by sbe_codec.hip inside its anonymous namespace, after order_select.hpp.
//
// The walk a poll of one Aeron image does over a raw block of a term buffer (the TermReader::read
// loop over 32-byte DataHeader frames), on the device (sbe_term_scan): which 32-byte slots of the
// block start a frame is a chain (frame k + 1 starts where frame k's aligned length says), and
// payload bytes may look exactly like headers, so only slots reachable from `start` count.
//
//   slot            32 bytes of block; a frame starts on a slot
//   successor       slot + align(frame_length, 32) / 32 for a frame that is consumed; a slot whose
//                   frame_length is <= 0 (UNCOMMITTED), 1..31 (SHORT) or runs past the block
//                   (PARTIAL, 64-bit arithmetic) stops the walk there and is not consumed
//   term_tile_chain one workgroup per tile of kTsSlots slots, one thread a slot: every slot's
//                   successor from its own first 8 bytes, clamped to the tile (a slot whose
//                   successor leaves the tile, or that stops, is its own successor: the tile's
//                   chains end in such a slot); pointer doubling in LDS (level k: the slot 2^k steps
//                   on, k = 0..9, with the sums over those steps) and one more composition of level
//                   9 with itself (1024 steps: a tile's chain has at most 1023) give, for every
//                   possible entry slot, the slot its chain ends in and the fragments and payload
//                   bytes it passes on the way; (exit, fragments, bytes) per entry go to the
//                   workspace.  The exit always lies outside the tile (or is a stop), so the walk
//                   across tiles visits a tile at most once
//   term_walk_tiles one lane follows entry -> exit from `start`: one step a tile visited, not a
//                   frame; it lists the visited tiles with their entry slot and fragment / byte
//                   bases, finds the tile the limit falls in, and writes counts for every stop but
//                   LIMIT
//   term_emit       one workgroup per visited tile: the doubling levels again, the slots reachable
//                   from the tile's entry marked with them from the top level down, a scan over the
//                   marked non-padding frames for each fragment's index and output offset; writes
//                   frag_off / flags / frag_src, copies the payloads (wave_copy16: the source is
//                   32-byte aligned, the destination is not), and in the limit tile the thread of
//                   the limit-th fragment writes counts (the walk stops behind that frame: a padding
//                   frame after it is not consumed)

constexpr uint32_t kTsSlots = 1024;                 // slots per tile (one thread each)
// Levels 0..9 kept in LDS: level k is 2^k steps on, so level 9 alone reaches 512 steps.  A tile's
// chain has at most kTsSlots - 1 = 1023 steps = 2^9 + ... + 2^0: marking from the top level down
// reaches every one of them, and the chain's end is level 9 applied twice (ts_levels).
constexpr uint32_t kTsLevels = 10;
static_assert((1u << kTsLevels) == kTsSlots, "two applications of the top level must cover a tile's longest chain");
constexpr uint32_t kTsTileBytes = 32 * kTsSlots;
constexpr uint32_t kTsStopBit = 0x80000000u;        // exit word: bit 31 stop, bits 28-30 reason, 0-27 slot
constexpr uint64_t kTsMaxBlock = 1ull << 30;

struct TsArgs {
    const uint8_t* block;
    uint64_t block_bytes;
    uint64_t start;
    uint64_t limit;      // min(fragment_limit, frag_capacity), >= 1
    uint8_t* out;        // or null
    uint64_t* frag_off;
    uint8_t* flags;
    uint32_t* frag_src;  // or null
    uint64_t* counts;
    uint32_t* w_exit;    // [tiles * kTsSlots] per entry slot: where its chain leaves the tile
    uint32_t* w_frags;   //                    fragments on the way
    uint32_t* w_bytes;   //                    their payload bytes
    uint4* visited;      // [tiles] tile, entry slot in it, fragment base, byte base
    uint32_t* nvisited;  // [1]
};

struct TsSlot {
    uint32_t exit;   // the successor (an absolute slot), or kTsStopBit | reason << 28 | this slot
    uint32_t pay;    // payload bytes of a consumed frame
    uint8_t flags;   // header byte 5
    bool frag;       // consumed and not a padding frame
};

// Slot g of the block, from its own first 8 bytes.
__device__ __forceinline__ TsSlot ts_slot(const TsArgs& a, uint32_t g) {
    TsSlot s{0u, 0u, 0, false};
    const uint64_t off = 32ull * g;
    if (off >= a.block_bytes) {
        s.exit = kTsStopBit | (SBE_TERM_STOP_END << 28) | g;
        return s;
    }
    const uint2 h = *reinterpret_cast<const uint2*>(a.block + off);
    const int32_t L = (int32_t)h.x;
    uint32_t stop = ~0u;
    uint64_t al = 0;
    if (L <= 0) stop = SBE_TERM_STOP_UNCOMMITTED;
    else if (L < 32) stop = SBE_TERM_STOP_SHORT;
    else {
        al = ((uint64_t)(uint32_t)L + 31ull) & ~31ull;
        if (off + al > a.block_bytes) stop = SBE_TERM_STOP_PARTIAL;
    }
    if (stop != ~0u) {
        s.exit = kTsStopBit | (stop << 28) | g;
        return s;
    }
    s.exit = g + (uint32_t)(al >> 5);  // <= block_bytes / 32 <= 2^25
    s.pay = (uint32_t)L - 32u;
    s.flags = (uint8_t)(h.y >> 8);
    s.frag = (h.y >> 16) != 0;
    return s;
}

struct TsLds {
    uint16_t jump[kTsLevels][kTsSlots];  // level k: the slot 2^k steps on (a chain's last slot is its own successor)
    uint32_t exit[kTsSlots];
    uint32_t pay[kTsSlots];              // payload bytes of the slot's own fragment (0 for padding and stops)
    uint32_t acc_b[kTsSlots];
    uint16_t acc_f[kTsSlots];
    uint8_t frag[kTsSlots];
    uint8_t mark[kTsSlots];
    uint32_t wave_f[kTsSlots / kWave], wave_b[kTsSlots / kWave];
};

// The doubling levels of tile t: L.jump[k][i] is the slot 2^k steps on from slot i, k = 0..9 (a
// chain's last slot is its own successor); s is the thread's own slot.  With kSums the sums over
// those steps are kept alongside, and the return value is the last slot of the chain from slot i,
// (f, b) the fragments and payload bytes of the frames before that last slot: level 9 reaches 512
// steps and a chain has up to 1023, so level 9 is applied once more to the slot it leads to, with
// that slot's 512-step sums added.  Without kSums (term_emit marks with the jump tables alone) the
// sums and two of the three barriers a level are left out, and the return value means nothing.
template <bool kSums>
__device__ __forceinline__ uint32_t ts_levels(const TsArgs& a, uint32_t t, TsLds& L, TsSlot& s, uint32_t& f, uint32_t& b) {
    const uint32_t i = threadIdx.x, base = t * kTsSlots;
    s = ts_slot(a, base + i);
    const bool last = (s.exit & kTsStopBit) || s.exit - base >= kTsSlots;
    L.jump[0][i] = (uint16_t)(last ? i : s.exit - base);
    f = (!last && s.frag) ? 1u : 0u;
    b = (!last && s.frag) ? s.pay : 0u;
    if (kSums) {
        L.exit[i] = s.exit;
        L.frag[i] = s.frag ? 1 : 0;
        L.pay[i] = s.frag ? s.pay : 0u;
        L.acc_f[i] = (uint16_t)f;
        L.acc_b[i] = b;
    }
    __syncthreads();
    for (uint32_t k = 1; k < kTsLevels; ++k) {
        const uint32_t j = L.jump[k - 1][i];
        L.jump[k][i] = L.jump[k - 1][j];
        if (kSums) {
            const uint32_t fj = L.acc_f[j], bj = L.acc_b[j];
            __syncthreads();
            f += fj;
            b += bj;
            L.acc_f[i] = (uint16_t)f;
            L.acc_b[i] = b;
        }
        __syncthreads();
    }
    if (!kSums) return 0u;
    // (f, b) and L.acc_* now cover 512 steps; the other up to 511 are those of the slot 512 steps on
    const uint32_t j = L.jump[kTsLevels - 1][i];
    f += L.acc_f[j];
    b += L.acc_b[j];
    return L.jump[kTsLevels - 1][j];
}

__global__ __launch_bounds__(kTsSlots) void term_tile_chain(TsArgs a, uint32_t tile0) {
    __shared__ TsLds L;
    const uint32_t t = tile0 + blockIdx.x, i = threadIdx.x;
    TsSlot s;
    uint32_t f, b;
    const uint32_t e = ts_levels<true>(a, t, L, s, f, b);  // a stop, or a frame whose successor leaves the tile
    const uint64_t g = (uint64_t)t * kTsSlots + i;
    a.w_exit[g] = L.exit[e];
    a.w_frags[g] = f + L.frag[e];  // a stop slot has frag = 0: it is not consumed
    a.w_bytes[g] = b + L.pay[e];
}

__global__ __launch_bounds__(kWave) void term_walk_tiles(TsArgs a) {
    if (threadIdx.x != 0) return;
    const uint64_t slots = a.block_bytes >> 5;
    uint64_t slot = a.start >> 5, frags = 0, bytes = 0;
    uint32_t nv = 0, stop;
    for (;;) {
        if (slot >= slots) {
            stop = SBE_TERM_STOP_END;
            break;
        }
        const uint32_t ex = a.w_exit[slot], f = a.w_frags[slot], b = a.w_bytes[slot];
        a.visited[nv++] = make_uint4((uint32_t)(slot / kTsSlots), (uint32_t)(slot % kTsSlots), (uint32_t)frags, (uint32_t)bytes);
        if (frags + f >= a.limit) {  // the limit-th fragment lies on this tile's chain: term_emit writes counts
            *a.nvisited = nv;
            return;
        }
        frags += f;
        bytes += b;
        if (ex & kTsStopBit) {
            stop = (ex >> 28) & 7u;
            slot = ex & 0x0fffffffu;
            break;
        }
        slot = ex;
    }
    *a.nvisited = nv;
    a.frag_off[frags] = bytes;
    a.counts[0] = frags;
    a.counts[1] = 32ull * slot;
    a.counts[2] = bytes;
    a.counts[3] = stop;
}

__global__ __launch_bounds__(kTsSlots) void term_emit(TsArgs a) {
    __shared__ TsLds L;
    if (blockIdx.x >= *a.nvisited) return;
    const uint4 v = a.visited[blockIdx.x];
    const uint32_t i = threadIdx.x, lane = i & (kWave - 1), w = i / kWave;
    TsSlot s;
    uint32_t f, b;
    L.mark[i] = i == v.y ? 1 : 0;
    ts_levels<false>(a, v.x, L, s, f, b);
    // levels 9..0 from the entry: every distance 0..1023 is a sum of distinct powers of two below 2^10
    for (int k = (int)kTsLevels - 1; k >= 0; --k) {
        if (L.mark[i]) L.mark[L.jump[k][i]] = 1;
        __syncthreads();
    }
    // the chain's fragments in slot order are in delivery order: successors only grow
    const bool take = L.mark[i] && s.frag;
    const uint64_t inc_f = wave_incl_scan64(take ? 1ull : 0ull, (int)lane);
    const uint64_t inc_b = wave_incl_scan64(take ? (uint64_t)s.pay : 0ull, (int)lane);
    if (lane == kWave - 1) {
        L.wave_f[w] = (uint32_t)inc_f;
        L.wave_b[w] = (uint32_t)inc_b;
    }
    __syncthreads();
    uint64_t idx = (uint64_t)v.z + inc_f - (take ? 1u : 0u), off = (uint64_t)v.w + inc_b - (take ? s.pay : 0u);
    for (uint32_t k = 0; k < kTsSlots / kWave; ++k) {
        idx += k < w ? L.wave_f[k] : 0u;
        off += k < w ? L.wave_b[k] : 0u;
    }
    const bool deliver = take && idx < a.limit;
    const uint64_t src = 32ull * ((uint64_t)v.x * kTsSlots + i);
    if (deliver) {
        a.frag_off[idx] = off;
        a.flags[idx] = s.flags;
        if (a.frag_src) a.frag_src[idx] = (uint32_t)src;
        if (idx + 1 == a.limit) {
            a.frag_off[idx + 1] = off + s.pay;
            a.counts[0] = a.limit;
            a.counts[1] = 32ull * s.exit;
            a.counts[2] = off + s.pay;
            a.counts[3] = SBE_TERM_STOP_LIMIT;
        }
    }
    if (!a.out) return;
    for (uint64_t mk = __ballot(deliver && s.pay != 0); mk; mk &= mk - 1) {
        const int k = __builtin_ctzll(mk);
        const uint64_t S = uniform64(__shfl(src, k, kWave)), D = uniform64(__shfl(off, k, kWave));
        const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(s.pay, k, kWave));
        wave_copy16(a.out + D, a.block + S + 32, n, (int)lane);
    }
}

// counts and frag_off[0] of a call that delivers nothing
__global__ void term_counts_only(uint64_t* counts, uint64_t* frag_off, uint64_t next, uint32_t stop) {
    counts[0] = 0;
    counts[1] = next;
    counts[2] = 0;
    counts[3] = stop;
    frag_off[0] = 0;
}
