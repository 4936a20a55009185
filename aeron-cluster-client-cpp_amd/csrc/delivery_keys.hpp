// delivery_keys.hpp — included by sbe_codec.hip inside its anonymous namespace, after json_paths.hpp.
//
// The keys the subscriber's callback looks up per record (examples/pubsub_reconnect_test.cpp:
// 625-691): result.message_id (view 2 of a parse-mode TopicMessage) and the client_order_id /
// order_id the callback reads out of the payload (:592-619), as byte ranges of the batch buffer
// that sbe_inflight_note_keys / sbe_inflight_lookup_keys take.  The ids come from an
// sbe_json_extract_batch over the nine paths of SBE_DLV_PATHS; the rule that picks among them is
// the callback's, line for line:
//   inner = message.message is an object:  client = str(2), order = str(3);
//                                          client empty and order_details (4) an object: client = str(5)
//   else message.order_details (6) is an object (the older format): client = str(7)
//   order empty: a non-empty str(8) (uuid) replaces it
// where str(p) is the member if it is a string and "" otherwise.  An escaped string (STRING_ESC)
// with a non-empty raw range decodes to a non-empty string, so it stops a fall-through like a
// plain one.  One launch, one lane per record, no workspace.

constexpr uint32_t kDkBlk = 256;
constexpr uint32_t kDkPaths = 9;

struct DkArgs {
    const uint64_t* rec_off;
    uint64_t n;
    const uint8_t* status;
    const uint32_t* view_off;
    const uint32_t* view_len;
    const uint8_t* select;  // or null: every TopicMessage
    const uint8_t* doc;
    const uint8_t* root_kind;
    const uint8_t* kind;
    const uint32_t* off;
    const uint32_t* len;
    uint64_t* msg_pos;
    uint32_t* msg_len;
    uint64_t* coid_pos;
    uint32_t* coid_len;
    uint8_t* coid_kind;
    uint64_t* oid_pos;
    uint32_t* oid_len;
    uint8_t* oid_kind;
    uint8_t* selected;
    uint64_t* totals;
};

struct DkStr {
    uint32_t kind, off, len;  // kind: SBE_JX_STRING, SBE_JX_STRING_ESC or SBE_JX_MISSING
};

__global__ __launch_bounds__(kDkBlk) void sbe_delivery_keys_kernel(DkArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kDkBlk + threadIdx.x;
    bool sel = false;
    int esc = 0;
    if (i < a.n) {
        const uint64_t b = a.rec_off[i], e = a.rec_off[i + 1];
        const uint64_t L64 = e > b ? e - b : 0;
        const uint32_t L = L64 > 0xffffffffull ? 0xffffffffu : (uint32_t)L64;
        // a range of the record, kept inside it whatever the descriptors say
        auto clamp = [&](uint32_t& o, uint32_t& l) {
            o = o <= L ? o : L;
            l = l <= L - o ? l : L - o;
        };
        sel = a.status[i] == SBE_ST_TM && (!a.select || a.select[i]);
        uint64_t mpos = b;
        uint32_t mlen = SBE_NO_KEY;
        DkStr client{SBE_JX_MISSING, 0, 0}, order{SBE_JX_MISSING, 0, 0};
        if (sel) {
            uint32_t vo = a.view_off[5 * i + 2], vl = a.view_len[5 * i + 2];
            clamp(vo, vl);
            if (vl) {  // :628, an empty message_id is not looked up
                mpos = b + vo;
                mlen = vl;
            }
            if (a.doc[i] == SBE_JX_OK && a.root_kind[i] == SBE_JX_OBJECT) {
                const uint8_t* kd = a.kind + kDkPaths * i;
                auto str = [&](uint32_t p) {  // find_str
                    const uint32_t k = kd[p];
                    if (k != SBE_JX_STRING && k != SBE_JX_STRING_ESC) return DkStr{SBE_JX_MISSING, 0, 0};
                    DkStr s{k, a.off[kDkPaths * i + p], a.len[kDkPaths * i + p]};
                    clamp(s.off, s.len);
                    return s;
                };
                const bool msg_obj = kd[0] == SBE_JX_OBJECT;
                if (msg_obj && kd[1] == SBE_JX_OBJECT) {
                    client = str(2);
                    order = str(3);
                    if (client.len == 0 && kd[4] == SBE_JX_OBJECT) client = str(5);
                } else if (msg_obj && kd[6] == SBE_JX_OBJECT) {
                    client = str(7);
                }
                if (order.len == 0) {
                    const DkStr u = str(8);
                    if (u.len) order = u;
                }
            }
        }
        a.msg_pos[i] = mpos;
        a.msg_len[i] = mlen;
        a.coid_pos[i] = client.len ? b + client.off : b;
        a.coid_len[i] = client.len ? client.len : SBE_NO_KEY;
        a.coid_kind[i] = (uint8_t)client.kind;
        a.oid_pos[i] = order.len ? b + order.off : b;
        a.oid_len[i] = order.len ? order.len : SBE_NO_KEY;
        a.oid_kind[i] = (uint8_t)order.kind;
        a.selected[i] = sel ? 1 : 0;
        esc = (client.kind == SBE_JX_STRING_ESC) + (order.kind == SBE_JX_STRING_ESC);
    }
    const int ns = __syncthreads_count(sel);
    const int n1 = __syncthreads_count(esc >= 1);
    const int n2 = __syncthreads_count(esc == 2);
    if (threadIdx.x == 0) {
        if (ns) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals), (unsigned long long)ns);
        if (n1 + n2) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals + 1), (unsigned long long)(n1 + n2));
    }
}
