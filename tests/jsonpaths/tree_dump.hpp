// TEST ONLY: the canonical dump of a parsed tree, shared by paths_ref.cpp and paths_pin.cpp (each
// includes it inside its anonymous namespace, behind its own Value and parse_from_stream), so that
// the two copies of the reader can be compared: every Value with its getOffsetStart(), its type
// and its content (reals as their bit pattern, object members in std::map order).
template <class V>
void dump_tree(const V& v, std::string& out) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "@%zu", v.tok_s);
    out += buf;
    switch (v.type) {
        case V::Null: out += 'n'; break;
        case V::Bool: out += v.b ? 't' : 'f'; break;
        case V::Int:
            std::snprintf(buf, sizeof buf, "i%lld", (long long)v.i);
            out += buf;
            break;
        case V::UInt:
            std::snprintf(buf, sizeof buf, "u%llu", (unsigned long long)v.u);
            out += buf;
            break;
        case V::Real: {
            uint64_t bits;
            std::memcpy(&bits, &v.d, 8);
            std::snprintf(buf, sizeof buf, "r%016llx", (unsigned long long)bits);
            out += buf;
            break;
        }
        case V::String:
            std::snprintf(buf, sizeof buf, "s%zu:", v.s.size());
            out += buf;
            out += v.s;
            break;
        case V::Array:
            out += '[';
            for (const V& x : v.arr) dump_tree(x, out);
            out += ']';
            break;
        case V::Object:
            out += '{';
            for (const auto& kv : v.obj) {
                std::snprintf(buf, sizeof buf, "%zu:", kv.first.size());
                out += buf;
                out += kv.first;
                dump_tree(kv.second, out);
            }
            out += '}';
            break;
    }
}

// verdict: 0 parsed, 1 parse returned false, 2 the stack-limit exception; the dump of a parsed
// tree goes to out[0, cap); returns its full length
template <class V>
uint64_t dump_document(const std::string& doc, uint32_t* verdict, char* out, uint64_t cap) {
    V root;
    std::string text;
    try {
        *verdict = parse_from_stream(doc, root) ? 0u : 1u;
    } catch (const std::runtime_error&) {
        *verdict = 2;
    }
    if (*verdict == 0) dump_tree(root, text);
    std::memcpy(out, text.data(), text.size() < cap ? text.size() : cap);
    return text.size();
}
