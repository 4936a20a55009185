// json_paths.hpp — included by sbe_codec.hip inside its anonymous namespace, after commit_class.hpp.
//
// sbe_json_extract_batch: the members a consumer's callback reads out of a decoded payload
// (examples/pubsub_reconnect_test.cpp:576-620: message.message.client_order_id, uuid, ...), for a
// caller-given table of member paths and every record of a batch in one launch.  The document is
// read as Json::parseFromStream with builder defaults reads it: the reader of seqnum.hpp (jtoken,
// jdecode_string, jnum_seq, the grammar and the stack limit of json_seq_eval / cm_doc_eval) with a
// third question asked of the walk.  The rules in the header of seqnum.hpp apply unchanged.
//
// The table is a trie built on the host (jx_build_trie): node 0 is the root, the children of a
// node have consecutive numbers, `below` is the set of paths at or below a node and `path` the
// path that ends at it.  A path resolves through objects only.  When a member name equal to a
// trie child is read, every path at or below that child goes back to MISSING before its value is
// read, so the last of several equal keys wins at every level (jsoncpp's operator[] on a name it
// already holds assigns to the same member).  Names are compared after decodeString.
//
// State of the walk, per lane: kind_bits (the stack limit needs them), the trie node of each open
// matched level packed into one 64-bit register (the root object and at most four containers under
// it), and how many of them are open.  A result is stored where it lands, in the record's row
// (kind / off / len of every path): the kernel keeps the rows of a tile in LDS and stores them
// coalesced at the end; nothing is returned through a struct of 16 entries (commit_class.hpp
// records what that cost).  The range of a container is opened with its '{' / '[' and closed when
// its level closes: the row holds its start, so no start is kept in the state.

constexpr uint32_t kJxMaxPaths = SBE_JSON_MAX_PATHS, kJxMaxDepth = SBE_JSON_MAX_DEPTH;
constexpr uint32_t kJxMaxName = SBE_JSON_MAX_NAME, kJxNameBytes = SBE_JSON_NAME_BYTES;
constexpr uint32_t kJxNodes = 68;  // the root and 16 x 4 nodes, rounded up to a multiple of 4
constexpr uint32_t kJxNoPath = 0xff;

struct JxTrie {
    uint8_t names[kJxNameBytes];
    uint16_t name_off[kJxNodes];
    uint16_t below[kJxNodes];      // bit p: path p ends at or below this node
    uint8_t name_len[kJxNodes];
    uint8_t first_child[kJxNodes];
    uint8_t n_child[kJxNodes];
    uint8_t path[kJxNodes];        // the path that ends here, or kJxNoPath
    uint32_t n_paths, n_nodes;
};
static_assert(sizeof(JxTrie) % 4 == 0 && sizeof(JxTrie) <= 1600, "the trie travels in the launch arguments");

// The caller's table as a trie; false: a value outside the design caps, an empty name or a duplicate path.
inline bool jx_build_trie(const sbe_json_paths* ps, JxTrie& T) {
    T = JxTrie{};
    if (!ps || !ps->depth || !ps->names || !ps->name_off) return false;
    const uint32_t P = ps->n_paths;
    if (P < 1 || P > kJxMaxPaths) return false;
    uint32_t first[kJxMaxPaths], tot = 0;
    for (uint32_t p = 0; p < P; ++p) {
        if (ps->depth[p] < 1 || ps->depth[p] > kJxMaxDepth) return false;
        first[p] = tot;
        tot += ps->depth[p];
    }
    for (uint32_t j = 0; j < tot; ++j) {
        if (ps->name_off[j + 1] <= ps->name_off[j] || ps->name_off[j + 1] - ps->name_off[j] > kJxMaxName) return false;
        if (ps->name_off[j + 1] - ps->name_off[0] > kJxNameBytes) return false;
    }
    uint16_t members[kJxNodes] = {};
    uint8_t level[kJxNodes] = {};
    uint32_t used = 0;  // bytes of T.names
    members[0] = (uint16_t)((1u << P) - 1);
    T.path[0] = kJxNoPath;
    T.n_nodes = 1;
    for (uint32_t q = 0; q < T.n_nodes; ++q) {
        const uint32_t d = level[q], fc = T.n_nodes;
        T.first_child[q] = (uint8_t)fc;
        for (uint32_t p = 0; p < P; ++p) {
            if (!((members[q] >> p) & 1) || ps->depth[p] <= d) continue;
            const uint8_t* nm = ps->names + ps->name_off[first[p] + d];
            const uint32_t nl = ps->name_off[first[p] + d + 1] - ps->name_off[first[p] + d];
            uint32_t c = fc;
            for (; c < T.n_nodes; ++c)
                if (T.name_len[c] == nl && std::memcmp(T.names + T.name_off[c], nm, nl) == 0) break;
            if (c == T.n_nodes) {
                ++T.n_nodes;
                T.name_off[c] = (uint16_t)used;
                T.name_len[c] = (uint8_t)nl;
                std::memcpy(T.names + used, nm, nl);
                used += nl;
                level[c] = (uint8_t)(d + 1);
                T.path[c] = kJxNoPath;
            }
            members[c] |= (uint16_t)(1u << p);
            if (ps->depth[p] == d + 1) {
                if (T.path[c] != kJxNoPath) return false;  // the same path twice
                T.path[c] = (uint8_t)p;
            }
        }
        T.n_child[q] = (uint8_t)(T.n_nodes - fc);
        T.below[q] = members[q];
    }
    T.n_paths = P;
    return true;
}

// One record's results: entry p of each array belongs to path p.
struct JxRow {
    uint8_t* kind;
    uint32_t* off;
    uint32_t* len;
};

// member name == the name of one of the children [fc, fc + count) of a node?  `alive` holds the
// children whose names agree with the bytes decoded so far.
struct JxKeySink {
    const JxTrie* T;
    uint32_t fc, alive, len = 0;
    __device__ __forceinline__ void put(uint32_t ch) {
        for (uint32_t m = alive; m; m &= m - 1) {
            const uint32_t j = (uint32_t)__builtin_ctz(m), c = fc + j;
            if (len >= T->name_len[c] || T->names[T->name_off[c] + len] != (uint8_t)ch) alive &= ~(1u << j);
        }
        ++len;
    }
    __device__ __forceinline__ uint32_t match() const {  // the child, or 0 (the root is nobody's child)
        for (uint32_t m = alive; m; m &= m - 1) {
            const uint32_t c = fc + (uint32_t)__builtin_ctz(m);
            if (T->name_len[c] == len) return c;
        }
        return 0;
    }
};

// The document walk of json_seq_eval / cm_doc_eval (same tokens, same grammar, same failures) with
// the path table as its question.  Returns SBE_JX_OK (root_kind: what the root is), SBE_JX_FAILED
// or SBE_JX_STACK; the row, which the caller hands over all MISSING, is all MISSING again after a
// failure.  base: the document's offset inside its record.
__device__ uint32_t jx_walk(const uint8_t* p, uint32_t n, const JxTrie& T, const JxRow& row, uint32_t base,
                            uint32_t& root_kind) {
    JCur c{p, n, 0};
    if (n >= 3 && p[0] == 0xEF && p[1] == 0xBB && p[2] == 0xBF) c.i = 3;  // skipBom
    uint64_t kind_bits[(kJsonStackLimit + 63) / 64];  // 1: object, 0: array, per open container
    int depth = 0;
    int mdepth = 0;      // the containers [0, mdepth) are matched levels: the root object, then values of trie nodes
    uint64_t nodes = 0;  // byte k: the trie node of level k
    uint32_t pend = 0;   // the trie node whose value comes next (0: none)
    uint32_t rk = SBE_JX_MISSING;
    uint32_t s, e;
    int t;
    enum { S_VALUE, S_KEY, S_OAFTER, S_AFIRST, S_AAFTER } st = S_VALUE;
    auto is_obj = [&](int dd) { return (kind_bits[dd >> 6] >> (dd & 63)) & 1; };
    auto push = [&](bool obj) {
        const uint64_t b = 1ull << (depth & 63);
        kind_bits[depth >> 6] = obj ? (kind_bits[depth >> 6] | b) : (kind_bits[depth >> 6] & ~b);
        ++depth;
    };
    auto set = [&](uint32_t node, uint32_t kind, uint32_t ts, uint32_t te) {
        const uint32_t q = T.path[node];
        if (q == kJxNoPath) return;
        row.kind[q] = (uint8_t)kind;
        row.off[q] = base + ts;
        row.len[q] = te - ts;
    };
    auto clear = [&](uint32_t mask) {
        for (; mask; mask &= mask - 1) {
            const uint32_t q = (uint32_t)__builtin_ctz(mask);
            row.kind[q] = SBE_JX_MISSING;
            row.off[q] = 0;
            row.len[q] = 0;
        }
    };
    auto fail = [&](uint32_t code) {
        clear((1u << T.n_paths) - 1);
        root_kind = SBE_JX_MISSING;
        return code;
    };
    auto close = [&](uint32_t end) {  // the innermost container ends at `end` (exclusive)
        if (depth == mdepth && mdepth > 0) {
            --mdepth;
            if (mdepth > 0) {
                const uint32_t q = T.path[(nodes >> (8 * mdepth)) & 0xff];
                if (q != kJxNoPath) row.len[q] = base + end - row.off[q];
            }
        }
        --depth;
    };
    for (;;) {
        bool value_done = false;
        if (st == S_VALUE || st == S_AFIRST) {
            if (st == S_AFIRST) {  // readArray: ']' right after '[' or ',' (spaces only)
                c.skip_spaces();
                if (c.i < c.n && c.p[c.i] == ']') {
                    ++c.i;
                    close(c.i);
                    value_done = true;
                }
            }
            if (!value_done) {
                if (depth >= kJsonStackLimit) return fail(SBE_JX_STACK);  // "Exceeded stackLimit in readValue()" (thrown)
                do t = jtoken(c, s, e);
                while (t == JT_COMMENT);
                const uint32_t what = pend;
                pend = 0;
                if (t == JT_OBEG || t == JT_ABEG) {
                    const bool obj = t == JT_OBEG;
                    if (depth == 0) {
                        rk = obj ? SBE_JX_OBJECT : SBE_JX_ARRAY;
                        if (obj) mdepth = 1;  // level 0: node 0
                    } else if (what) {  // depth == mdepth: the member was named in a matched level
                        set(what, obj ? SBE_JX_OBJECT : SBE_JX_ARRAY, s, s);
                        nodes = (nodes & ~(0xffull << (8 * mdepth))) | ((uint64_t)what << (8 * mdepth));
                        ++mdepth;
                    }
                    push(obj);
                    st = obj ? S_KEY : S_AFIRST;
                    continue;
                }
                uint32_t kind, ts = s, te = e;
                if (t == JT_NUM) {
                    uint64_t v;
                    if (!jnum_seq(p, s, e, v)) return fail(SBE_JX_FAILED);
                    kind = SBE_JX_NUMBER;
                } else if (t == JT_STR) {
                    NullSink k;
                    if (!jdecode_string(p, s, e, k)) return fail(SBE_JX_FAILED);
                    kind = SBE_JX_STRING;
                    ts = s + 1;
                    te = e - 1;
                    if (what || depth == 0)
                        for (uint32_t j = ts; j < te; ++j)
                            if (p[j] == '\\') kind = SBE_JX_STRING_ESC;
                } else if (t == JT_LIT) {
                    kind = p[s] == 't' ? SBE_JX_TRUE : p[s] == 'f' ? SBE_JX_FALSE : SBE_JX_NULL;
                } else {
                    return fail(SBE_JX_FAILED);  // "Syntax error: value, object or array expected."
                }
                if (depth == 0) rk = kind;
                else if (what) set(what, kind, ts, te);
                value_done = true;
            }
        } else if (st == S_KEY) {  // member name, or '}' (empty object / trailing comma)
            do t = jtoken(c, s, e);
            while (t == JT_COMMENT);
            if (t == JT_OEND) {
                close(e);
                value_done = true;
            } else {
                if (t != JT_STR) return fail(SBE_JX_FAILED);
                const uint32_t lv = depth == mdepth ? (uint32_t)((nodes >> (8 * (mdepth - 1))) & 0xff) : 0u;
                const uint32_t nc = depth == mdepth ? T.n_child[lv] : 0u;
                if (nc) {
                    JxKeySink k{&T, T.first_child[lv], (1u << nc) - 1};
                    if (!jdecode_string(p, s, e, k)) return fail(SBE_JX_FAILED);
                    pend = k.match();
                    if (pend) clear(T.below[pend]);  // the member is named (again): what it held is gone
                } else {
                    NullSink k;
                    if (!jdecode_string(p, s, e, k)) return fail(SBE_JX_FAILED);
                }
                if (jtoken(c, s, e) != JT_COLON) return fail(SBE_JX_FAILED);  // "Missing ':' after object member name"
                st = S_VALUE;
                continue;
            }
        } else if (st == S_OAFTER) {  // ',' or '}'; after comments, the next token stands as separator
            t = jtoken(c, s, e);
            if (t != JT_OEND && t != JT_COMMA && t != JT_COMMENT) return fail(SBE_JX_FAILED);  // "Missing ',' or '}' ..."
            while (t == JT_COMMENT) t = jtoken(c, s, e);
            if (t == JT_OEND) {
                close(e);
                value_done = true;
            } else {
                st = S_KEY;
                continue;
            }
        } else {  // S_AAFTER
            do t = jtoken(c, s, e);
            while (t == JT_COMMENT);
            if (t == JT_AEND) {
                close(e);
                value_done = true;
            } else {
                if (t != JT_COMMA) return fail(SBE_JX_FAILED);  // "Missing ',' or ']' in array declaration"
                st = S_AFIRST;
                continue;
            }
        }
        if (value_done) {
            if (depth == 0) break;  // the root is complete; what follows is ignored
            st = is_obj(depth - 1) ? S_OAFTER : S_AAFTER;
        }
    }
    root_kind = rk;
    return SBE_JX_OK;
}

#ifndef SEQNUM_HOST_CHECK  // tests/jsonpaths/paths_host_check.cpp compiles the code above for the host
struct JxArgs {
    const uint8_t* in;
    const uint64_t* rec_off;
    uint64_t n;
    const uint8_t* status;  // null: every record is its own document
    const uint8_t* flags;
    const uint32_t* view_off;
    const uint32_t* view_len;
    const uint8_t* select;  // null: every record
    uint32_t view;
    uint8_t* doc;
    uint8_t* root_kind;
    uint8_t* kind;
    uint32_t* off;
    uint32_t* len;
    JxTrie trie;
};
static_assert(sizeof(JxArgs) <= 2048, "launch arguments");

constexpr uint32_t kJxWin = 16384;         // LDS window of a tile, bytes
constexpr uint32_t kJxLong = kJxWin - 16;  // longer documents are read from HBM
constexpr uint32_t kJxRowBytes = 9;        // kind, off, len of one path

// One wave per 64-record tile, one lane per record (the shape of sbe_commit_kernel).  Dynamic LDS:
// the tile's result rows, off [64 P], len [64 P], kind [64 P].
__global__ __launch_bounds__(kWave) void sbe_json_extract_kernel(JxArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kJxWin + 16];
    __shared__ JxTrie trie;
    extern __shared__ __attribute__((aligned(16))) uint8_t jx_rows[];
    const int lane = threadIdx.x;
    const uint32_t P = a.trie.n_paths;
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile, r = t0 + lane;
    const bool valid = r < a.n;
    uint32_t* const roff = reinterpret_cast<uint32_t*>(jx_rows);
    uint32_t* const rlen = roff + kTile * P;
    uint8_t* const rkind = reinterpret_cast<uint8_t*>(rlen + kTile * P);
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&a.trie);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&trie);
        for (uint32_t j = lane; j < sizeof(JxTrie) / 4; j += kWave) dst[j] = src[j];
        for (uint32_t j = lane; j < kTile * P * kJxRowBytes / 4; j += kWave) roff[j] = 0;  // every path MISSING
    }
    __syncthreads();

    uint64_t ds = 0;   // the document's first byte in `in`
    uint32_t dl = 0, vo = 0;
    uint32_t code = SBE_JX_NOT_SELECTED, rk = SBE_JX_MISSING;
    bool pending = false;
    if (valid && (!a.select || a.select[r]) && (!a.status || a.status[r] == SBE_ST_TM)) {
        const uint64_t b = a.rec_off[r], e = a.rec_off[r + 1];
        const uint64_t L64 = e > b ? e - b : 0;
        const uint32_t L = L64 > 0xffffffffull ? 0xffffffffu : (uint32_t)L64;
        dl = L;
        if (a.status) {  // the view, kept inside the record whatever the descriptors say
            const uint32_t o = a.view_off[5 * r + a.view], l = a.view_len[5 * r + a.view];
            vo = o <= L ? o : L;
            dl = l <= L - vo ? l : L - vo;
            if (a.view == 4 && (a.flags[r] & SBE_FL_HEADERS_E100)) dl = 0;
        }
        ds = b + vo;
        code = SBE_JX_EMPTY;
        pending = dl != 0;
    }
    const JxRow row{rkind + lane * P, roff + lane * P, rlen + lane * P};
    // documents longer than the window: read from HBM (as decode's long records are)
    if (pending && dl > kJxLong) {
        code = jx_walk(a.in + ds, dl, trie, row, vo, rk);
        pending = false;
    }
    while (__ballot(pending)) {
        const uint64_t ws = cm_wave_min64(pending ? ds : ~0ull), we = cm_wave_max64(pending ? ds + dl : 0ull);
        const uint8_t* p0 = a.in + ws;
        const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(p0) & 15u);
        const uint8_t* base = p0 - lead;  // 16-B aligned; every chunk read below holds a byte of [ws, we)
        const uint64_t span = (uint64_t)lead + (we - ws);
        const uint32_t nbytes = span < kJxWin ? (uint32_t)span : kJxWin;
        const uint32_t nch = (nbytes + 15) >> 4;
        typedef uint32_t jx_u32x4 __attribute__((ext_vector_type(4)));
        for (uint32_t c = lane; c < nch; c += kWave)
            *reinterpret_cast<jx_u32x4*>(win + 16 * c) =
                __builtin_nontemporal_load(reinterpret_cast<const jx_u32x4*>(base) + c);
        __syncthreads();
        const uint64_t o0 = (uint64_t)lead + (ds - ws);
        if (pending && o0 + dl <= nbytes) {
            code = jx_walk(win + (uint32_t)o0, dl, trie, row, vo, rk);
            pending = false;
        }
        __syncthreads();
    }
    __syncthreads();
    if (valid) {
        a.doc[r] = (uint8_t)code;
        a.root_kind[r] = (uint8_t)rk;
    }
    const uint64_t left = a.n - t0;
    const uint32_t cnt = (uint32_t)(left < kTile ? left : kTile) * P;
    const uint64_t o = t0 * P;
    for (uint32_t j = lane; j < cnt; j += kWave) {
        a.kind[o + j] = rkind[j];
        a.off[o + j] = roff[j];
        a.len[o + j] = rlen[j];
    }
}
#endif
