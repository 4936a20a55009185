// TEST ONLY: an independent restatement of what sbe_json_extract_batch computes, for its tests.
// Where the device code walks a document as a stream of tokens and keeps only what the path table
// asks for, this one builds the whole tree (a recursive reader with the semantics of jsoncpp
// 1.9.5's OurReader under CharReaderBuilder defaults, function by function: the reader of
// tests/autocommit/commit_ref.cpp, copied, with jsoncpp's getOffsetStart() / getOffsetLimit() kept
// on every Value) and then resolves each path on the tree with isObject / isMember / operator[],
// as examples/pubsub_reconnect_test.cpp:576-620 and src/commit_manager.cpp:177-195 do.  jsoncpp
// itself is not available to the tests: this copy is pinned to the older one (paths_pin.cpp: the
// same verdict and the same canonical dump of the tree on every document of a CPU test), which is
// pinned to the project's oracle in turn.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sbecodec.h"

namespace {

struct Value {
    enum Type { Null, Int, UInt, Real, String, Bool, Array, Object } type = Null;
    int64_t i = 0;
    uint64_t u = 0;
    double d = 0;
    bool b = false;
    std::string s;
    std::vector<Value> arr;
    std::map<std::string, Value> obj;
    // getOffsetStart() / getOffsetLimit(): the token (strings: with the quotes), a container from
    // its opening bracket to behind its closing one
    size_t tok_s = 0, tok_e = 0;

    bool isMember(const std::string& key) const {  // JSON_ASSERT_MESSAGE: null or object, else throws
        if (type == Null) return false;
        if (type != Object) throw std::logic_error("isMember: not an object");
        return obj.count(key) != 0;
    }
    const Value& operator[](const std::string& key) const {
        static const Value null_value;
        if (type == Null) return null_value;
        if (type != Object) throw std::logic_error("operator[]: not an object");
        auto it = obj.find(key);
        return it == obj.end() ? null_value : it->second;
    }
    bool isObject() const { return type == Object; }
};

class Reader {
public:
    enum Tok { EndOfStream, ObjectBegin, ObjectEnd, ArrayBegin, ArrayEnd, Str, Number, True, False, NullTok,
               ArraySeparator, MemberSeparator, Comment, Error };
    struct Token {
        Tok type;
        size_t start, end;
    };
    explicit Reader(const std::string& doc) : doc_(doc), cur_(0), end_(doc.size()) {}

    bool parse(Value& root) {  // OurReader::parse; throws on the stack limit
        if (end_ - cur_ >= 3 && doc_.compare(0, 3, "\xEF\xBB\xBF") == 0) cur_ += 3;  // skipBom
        depth_ = 0;
        return readValue(root);  // failIfExtra is off: what follows the root is not looked at
    }

private:
    const std::string& doc_;
    size_t cur_, end_;
    int depth_ = 0;

    int getNextChar() { return cur_ == end_ ? 0 : (unsigned char)doc_[cur_++]; }
    void skipSpaces() {
        while (cur_ != end_) {
            const char c = doc_[cur_];
            if (c == ' ' || c == '\t' || c == '\r' || c == '\n') ++cur_;
            else break;
        }
    }
    bool match(const char* pat, size_t n) {
        if (end_ - cur_ < n) return false;
        if (doc_.compare(cur_, n, pat) != 0) return false;
        cur_ += n;
        return true;
    }
    bool readString() {
        int c = 0;
        while (cur_ != end_) {
            c = getNextChar();
            if (c == '\\') getNextChar();
            else if (c == '"') break;
        }
        return c == '"';
    }
    bool readCStyleComment() {
        while (cur_ + 1 < end_) {
            const int c = getNextChar();
            if (c == '*' && doc_[cur_] == '/') break;
        }
        return getNextChar() == '/';
    }
    bool readCppStyleComment() {
        while (cur_ != end_) {
            const int c = getNextChar();
            if (c == '\n') break;
            if (c == '\r') {
                if (cur_ != end_ && doc_[cur_] == '\n') getNextChar();
                break;
            }
        }
        return true;
    }
    bool readComment() {
        const int c = getNextChar();
        if (c == '*') return readCStyleComment();
        if (c == '/') return readCppStyleComment();
        return false;
    }
    bool readNumber(bool checkInf) {
        size_t p = cur_;
        if (checkInf && p != end_ && doc_[p] == 'I') {
            cur_ = ++p;
            return false;
        }
        char c = '0';
        auto next = [&] { c = (cur_ = p) < end_ ? doc_[p++] : '\0'; };
        while (c >= '0' && c <= '9') next();
        if (c == '.') {
            next();
            while (c >= '0' && c <= '9') next();
        }
        if (c == 'e' || c == 'E') {
            next();
            if (c == '+' || c == '-') next();
            while (c >= '0' && c <= '9') next();
        }
        return true;
    }
    bool readToken(Token& t) {
        skipSpaces();
        t.start = cur_;
        const int c = getNextChar();
        bool ok = true;
        switch (c) {
            case '{': t.type = ObjectBegin; break;
            case '}': t.type = ObjectEnd; break;
            case '[': t.type = ArrayBegin; break;
            case ']': t.type = ArrayEnd; break;
            case '"': t.type = Str; ok = readString(); break;
            case '/': t.type = Comment; ok = readComment(); break;
            case '0': case '1': case '2': case '3': case '4': case '5': case '6': case '7': case '8': case '9':
                t.type = Number;
                readNumber(false);
                break;
            case '-':
                if (readNumber(true)) t.type = Number;
                else ok = false;  // -Infinity needs allowSpecialFloats
                break;
            case 't': t.type = True; ok = match("rue", 3); break;
            case 'f': t.type = False; ok = match("alse", 4); break;
            case 'n': t.type = NullTok; ok = match("ull", 3); break;
            case ',': t.type = ArraySeparator; break;
            case ':': t.type = MemberSeparator; break;
            case 0: t.type = EndOfStream; break;
            default: ok = false; break;  // single quotes, NaN, Infinity: off by default
        }
        if (!ok) t.type = Error;
        t.end = cur_;
        return ok;
    }

    bool readValue(Value& v) {
        if (depth_ + 1 > 1000) throw std::runtime_error("Exceeded stackLimit in readValue().");
        Token t;
        do readToken(t);
        while (t.type == Comment);  // skipCommentTokens
        v = Value();
        v.tok_s = t.start;
        v.tok_e = t.end;
        switch (t.type) {
            case ObjectBegin: {
                const bool ok = readObject(v);
                v.tok_e = cur_;  // setOffsetLimit(current_ - begin_): behind the closing bracket
                return ok;
            }
            case ArrayBegin: {
                const bool ok = readArray(v);
                v.tok_e = cur_;
                return ok;
            }
            case Number: return decodeNumber(t, v);
            case Str:
                v.type = Value::String;
                return decodeString(t, v.s);
            case True: v.type = Value::Bool; v.b = true; return true;
            case False: v.type = Value::Bool; v.b = false; return true;
            case NullTok: return true;
            default: return false;  // "Syntax error: value, object or array expected."
        }
    }
    bool readObject(Value& v) {
        v.type = Value::Object;
        Token name_tok;
        std::string name;
        while (readToken(name_tok)) {
            bool ok = true;
            while (name_tok.type == Comment && ok) ok = readToken(name_tok);
            if (!ok) break;
            if (name_tok.type == ObjectEnd) return true;  // empty object or trailing comma (allowed)
            name.clear();
            if (name_tok.type != Str) break;  // numeric keys: off by default
            if (!decodeString(name_tok, name)) return false;
            Token colon;
            if (!readToken(colon) || colon.type != MemberSeparator) return false;
            Value& slot = v.obj[name];  // a duplicate key names the member again; its value is replaced
            ++depth_;
            ok = readValue(slot);
            --depth_;
            if (!ok) return false;
            Token comma;
            if (!readToken(comma) || (comma.type != ObjectEnd && comma.type != ArraySeparator && comma.type != Comment))
                return false;  // "Missing ',' or '}' in object declaration"
            bool fin = true;
            while (comma.type == Comment && fin) fin = readToken(comma);
            if (comma.type == ObjectEnd) return true;
        }
        return false;  // "Missing '}' or object member name"
    }
    bool readArray(Value& v) {
        v.type = Value::Array;
        for (;;) {
            skipSpaces();
            if (cur_ != end_ && doc_[cur_] == ']') {  // empty array, or trailing comma (allowed)
                Token t;
                readToken(t);
                return true;
            }
            v.arr.emplace_back();
            ++depth_;
            // emplace_back may have moved the elements: take the reference after it
            bool ok = readValue(v.arr.back());
            --depth_;
            if (!ok) return false;
            Token t;
            ok = readToken(t);
            while (t.type == Comment && ok) ok = readToken(t);
            if (!ok || (t.type != ArraySeparator && t.type != ArrayEnd)) return false;
            if (t.type == ArrayEnd) break;
        }
        return true;
    }
    bool decodeNumber(const Token& t, Value& v) {
        size_t p = t.start;
        const bool neg = doc_[p] == '-';
        if (neg) ++p;
        const uint64_t maxv = neg ? (uint64_t)1 << 63 : ~0ull, thr = maxv / 10;
        uint64_t val = 0;
        while (p < t.end) {
            const char c = doc_[p++];
            if (c < '0' || c > '9') return decodeDouble(t, v);
            const uint64_t dg = c - '0';
            if (val >= thr) {
                if (val > thr || p != t.end || dg > maxv % 10) return decodeDouble(t, v);
            }
            val = val * 10 + dg;
        }
        if (neg) {
            v.type = Value::Int;
            v.i = (int64_t)(0 - val);
        } else if (val <= (uint64_t)INT64_MAX) {
            v.type = Value::Int;
            v.i = (int64_t)val;
        } else {
            v.type = Value::UInt;
            v.u = val;
        }
        return true;
    }
    // istringstream >> double: the whole token must convert; an overflow becomes +-infinity
    bool decodeDouble(const Token& t, Value& v) {
        const std::string tok = doc_.substr(t.start, t.end - t.start);
        char* endp = nullptr;
        const double d = strtod(tok.c_str(), &endp);
        if (tok.empty() || endp != tok.c_str() + tok.size()) return false;  // "'...' is not a number."
        v.type = Value::Real;
        v.d = d;
        return true;
    }
    static void utf8(uint32_t cp, std::string& out) {
        if (cp <= 0x7f) {
            out += (char)cp;
        } else if (cp <= 0x7ff) {
            out += (char)(0xC0 | (cp >> 6));
            out += (char)(0x80 | (cp & 0x3f));
        } else if (cp <= 0xffff) {
            out += (char)(0xE0 | (cp >> 12));
            out += (char)(0x80 | ((cp >> 6) & 0x3f));
            out += (char)(0x80 | (cp & 0x3f));
        } else if (cp <= 0x10ffff) {
            out += (char)(0xF0 | (cp >> 18));
            out += (char)(0x80 | ((cp >> 12) & 0x3f));
            out += (char)(0x80 | ((cp >> 6) & 0x3f));
            out += (char)(0x80 | (cp & 0x3f));
        }
    }
    bool escapeSequence(size_t& p, size_t end, uint32_t& cp) {
        if (end - p < 4) return false;
        cp = 0;
        for (int k = 0; k < 4; ++k) {
            const char c = doc_[p++];
            cp *= 16;
            if (c >= '0' && c <= '9') cp += c - '0';
            else if (c >= 'a' && c <= 'f') cp += c - 'a' + 10;
            else if (c >= 'A' && c <= 'F') cp += c - 'A' + 10;
            else return false;
        }
        return true;
    }
    bool codePoint(size_t& p, size_t end, uint32_t& cp) {
        if (!escapeSequence(p, end, cp)) return false;
        if (cp >= 0xD800 && cp <= 0xDBFF) {
            if (end - p < 6) return false;
            if (doc_[p++] == '\\' && doc_[p++] == 'u') {
                uint32_t lo;
                if (!escapeSequence(p, end, lo)) return false;
                cp = 0x10000 + ((cp & 0x3FF) << 10) + (lo & 0x3FF);
            } else {
                return false;
            }
        }
        return true;
    }
    bool decodeString(const Token& t, std::string& out) {
        out.clear();
        size_t p = t.start + 1;
        const size_t end = t.end - 1;
        while (p != end) {
            const char c = doc_[p++];
            if (c == '"') break;
            if (c != '\\') {
                out += c;
                continue;
            }
            if (p == end) return false;  // "Empty escape sequence in string"
            const char x = doc_[p++];
            switch (x) {
                case '"': out += '"'; break;
                case '/': out += '/'; break;
                case '\\': out += '\\'; break;
                case 'b': out += '\b'; break;
                case 'f': out += '\f'; break;
                case 'n': out += '\n'; break;
                case 'r': out += '\r'; break;
                case 't': out += '\t'; break;
                case 'u': {
                    uint32_t cp;
                    if (!codePoint(p, end, cp)) return false;
                    utf8(cp, out);
                    break;
                }
                default: return false;  // "Bad escape sequence in string"
            }
        }
        return true;
    }
};

// Json::parseFromStream(builder, stream, &root, &errors); the stack-limit exception propagates
bool parse_from_stream(const std::string& doc, Value& root) {
    Reader r(doc);
    return r.parse(root);
}

#include "tree_dump.hpp"

// kind / range of one resolved Value, as the interface reports them (range relative to the document)
void describe(const Value& v, const std::string& doc, uint8_t& kind, uint32_t& off, uint32_t& len) {
    size_t s = v.tok_s, e = v.tok_e;
    switch (v.type) {
        case Value::String:
            ++s;
            --e;
            kind = doc.find('\\', s) < e ? SBE_JX_STRING_ESC : SBE_JX_STRING;
            break;
        case Value::Bool: kind = v.b ? SBE_JX_TRUE : SBE_JX_FALSE; break;
        case Value::Null: kind = SBE_JX_NULL; break;
        case Value::Object: kind = SBE_JX_OBJECT; break;
        case Value::Array: kind = SBE_JX_ARRAY; break;
        default: kind = SBE_JX_NUMBER; break;
    }
    off = (uint32_t)s;
    len = (uint32_t)(e - s);
}

// ---- Value's conversions (jsoncpp 1.9.5 json_value.cpp / json_writer.cpp) ----
std::string value_to_string(double value) {  // valueToString(double, false, 17, significantDigits)
    if (!std::isfinite(value)) return std::isnan(value) ? "null" : value < 0 ? "-1e+9999" : "1e+9999";
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.*g", 17, value);
    std::string s(buf);
    if (s.find('.') == std::string::npos && s.find('e') == std::string::npos) s += ".0";
    return s;
}
std::string as_string(const Value& v) {
    switch (v.type) {
        case Value::Null: return "";
        case Value::String: return v.s;
        case Value::Bool: return v.b ? "true" : "false";
        case Value::Int: return std::to_string((long long)v.i);
        case Value::UInt: return std::to_string((unsigned long long)v.u);
        case Value::Real: return value_to_string(v.d);
        default: throw std::runtime_error("Type is not convertible to string");
    }
}
uint64_t as_uint64(const Value& v) {
    switch (v.type) {
        case Value::Int:
            if (v.i < 0) throw std::runtime_error("LargestInt out of UInt64 range");
            return (uint64_t)v.i;
        case Value::UInt: return v.u;
        case Value::Real:  // the interface's rule: a real in [0, 2^64), truncated
            if (!(v.d >= 0.0 && v.d < 18446744073709551616.0)) throw std::runtime_error("double out of UInt64 range");
            return (uint64_t)v.d;
        case Value::Null: return 0;
        case Value::Bool: return v.b ? 1 : 0;
        default: throw std::runtime_error("Value is not convertible to UInt64.");
    }
}
// Value::get(key, default): the member, or the default; requires an object or null
Value get(const Value& root, const std::string& key, const Value& dflt) {
    if (root.type != Value::Null && root.type != Value::Object)
        throw std::runtime_error("in Json::Value::find(begin, end): requires objectValue or nullValue");
    if (root.type == Value::Null) return dflt;
    auto it = root.obj.find(key);
    return it == root.obj.end() ? dflt : it->second;
}

// ---- the subscriber callback's body, examples/pubsub_reconnect_test.cpp:582-623 ----
void order_ids(const std::string& payload, std::string& extracted_client_order_id, std::string& extracted_order_id) {
    extracted_client_order_id.clear();
    extracted_order_id.clear();
    try {
        if (!payload.empty()) {
            Value root;
            if (parse_from_stream(payload, root)) {
                auto find_str = [](const Value& obj, const char* key) -> std::string {
                    return obj.isMember(key) && obj[key].type == Value::String ? as_string(obj[key]) : "";
                };
                const Value null_value;
                const Value& msg = root.isMember("message") ? root["message"] : null_value;
                const Value& inner = (msg.isObject() && msg.isMember("message")) ? msg["message"] : null_value;
                if (inner.isObject()) {
                    extracted_client_order_id = find_str(inner, "client_order_id");
                    extracted_order_id = find_str(inner, "order_id");
                    if (extracted_client_order_id.empty() && inner.isMember("order_details") &&
                        inner["order_details"].isObject()) {
                        extracted_client_order_id = find_str(inner["order_details"], "client_order_id");
                    }
                } else if (msg.isObject() && msg.isMember("order_details") && msg["order_details"].isObject()) {
                    extracted_client_order_id = find_str(msg["order_details"], "client_order_id");
                }
                if (extracted_order_id.empty()) {
                    std::string maybe_uuid = find_str(root, "uuid");
                    if (!maybe_uuid.empty()) extracted_order_id = maybe_uuid;
                }
            }
        }
    } catch (...) {  // the example drops both on anything thrown
        extracted_client_order_id.clear();
        extracted_order_id.clear();
    }
}

// ---- CommitManager::parse_commit_offset, src/commit_manager.cpp:177-195 ----
struct CommitOffset {
    std::string topic, message_identifier, message_id;
    uint64_t timestamp_nanos = 0, sequence_number = 0;
};
CommitOffset parse_commit_offset(const std::string& payload) {
    Value root;
    if (!parse_from_stream(payload, root)) throw std::runtime_error("Failed to parse commit offset JSON: ");
    Value empty_string, zero;
    empty_string.type = Value::String;
    zero.type = Value::Int;
    CommitOffset offset;
    offset.topic = as_string(get(root, "topic", empty_string));
    offset.message_identifier = as_string(get(root, "message_identifier", empty_string));
    offset.message_id = as_string(get(root, "message_id", empty_string));
    offset.timestamp_nanos = as_uint64(get(root, "timestamp_nanos", zero));
    offset.sequence_number = as_uint64(get(root, "sequence_number", zero));
    return offset;
}

size_t put(const std::string& s, char* out, uint64_t cap) {
    std::memcpy(out, s.data(), s.size() < cap ? s.size() : cap);
    return s.size();
}

}  // namespace

extern "C" {

// the order-id rule on one payload: both strings into out (back to back), their lengths in len[2]
void pref_order_ids(const uint8_t* p, uint64_t n, char* out, uint64_t cap, uint64_t* len) {
    std::string a, b;
    order_ids(std::string(reinterpret_cast<const char*>(p), n), a, b);
    len[0] = put(a, out, cap);
    len[1] = put(b, out + (len[0] < cap ? len[0] : cap), cap - (len[0] < cap ? len[0] : cap));
}

// parse_commit_offset on one document: 0 and the five members (three strings back to back, lens[3],
// nums[2]), 1 the parse failure's exception, 2 any other exception
int pref_parse_commit_offset(const uint8_t* p, uint64_t n, char* out, uint64_t cap, uint64_t* lens, uint64_t* nums) {
    try {
        const CommitOffset o = parse_commit_offset(std::string(reinterpret_cast<const char*>(p), n));
        const std::string all = o.topic + o.message_identifier + o.message_id;
        put(all, out, cap);
        lens[0] = o.topic.size();
        lens[1] = o.message_identifier.size();
        lens[2] = o.message_id.size();
        nums[0] = o.timestamp_nanos;
        nums[1] = o.sequence_number;
        return 0;
    } catch (const std::exception& e) {
        return std::strncmp(e.what(), "Failed to parse commit offset JSON: ", 36) == 0 ? 1 : 2;
    }
}

// asString / asUInt64 of the root member `key` of one parsed document (Value::get's null when it
// is absent): codes 0 converted, 1 throws; -1 when the document does not parse to an object
int pref_convert(const uint8_t* p, uint64_t n, const char* key, int* s_code, char* out, uint64_t cap, uint64_t* s_len,
                 int* u_code, uint64_t* u_val) {
    Value root;
    try {
        if (!parse_from_stream(std::string(reinterpret_cast<const char*>(p), n), root) || !root.isObject()) return -1;
    } catch (const std::exception&) {
        return -1;
    }
    const Value v = get(root, key, Value());
    try {
        *s_len = put(as_string(v), out, cap);
        *s_code = 0;
    } catch (const std::exception&) {
        *s_code = 1;
    }
    try {
        *u_val = as_uint64(v);
        *u_code = 0;
    } catch (const std::exception&) {
        *u_code = 1;
    }
    return 0;
}

}  // extern "C"

extern "C" {

// verdict (0 parsed, 1 parse returned false, 2 the stack-limit exception) and the canonical dump
// of the tree (tree_dump.hpp) into out[0, cap); returns the dump's length
uint64_t pref_dump(const uint8_t* p, uint64_t n, uint32_t* verdict, char* out, uint64_t cap) {
    return dump_document<Value>(std::string(reinterpret_cast<const char*>(p), n), verdict, out, cap);
}

// The arguments of sbe_json_extract_batch, in host memory (status == NULL: bare documents).
void pref_extract(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const uint8_t* status, const uint8_t* flags,
                  const uint32_t* view_off, const uint32_t* view_len, uint32_t view, const uint8_t* select,
                  uint32_t n_paths, const uint8_t* depth, const uint8_t* names, const uint32_t* name_off, uint8_t* doc,
                  uint8_t* root_kind, uint8_t* kind, uint32_t* off, uint32_t* len) {
    std::vector<std::vector<std::string>> paths(n_paths);
    for (uint32_t p = 0, j = 0; p < n_paths; ++p)
        for (uint32_t k = 0; k < depth[p]; ++k, ++j)
            paths[p].emplace_back(reinterpret_cast<const char*>(names) + name_off[j], name_off[j + 1] - name_off[j]);
    for (uint64_t i = 0; i < n; ++i) {
        doc[i] = SBE_JX_NOT_SELECTED;
        root_kind[i] = SBE_JX_MISSING;
        for (uint32_t p = 0; p < n_paths; ++p) {
            kind[i * n_paths + p] = SBE_JX_MISSING;
            off[i * n_paths + p] = len[i * n_paths + p] = 0;
        }
        if (select && !select[i]) continue;
        if (status && status[i] != SBE_ST_TM) continue;
        const uint64_t L = rec_off[i + 1] > rec_off[i] ? rec_off[i + 1] - rec_off[i] : 0;
        uint64_t vo = 0, vl = L;
        if (status) {  // the view, kept inside its record
            vo = view_off[5 * i + view] <= L ? view_off[5 * i + view] : L;
            vl = view_len[5 * i + view] <= L - vo ? view_len[5 * i + view] : L - vo;
            if (view == 4 && (flags[i] & SBE_FL_HEADERS_E100)) vl = 0;
        }
        const std::string text(reinterpret_cast<const char*>(in) + rec_off[i] + vo, vl);
        if (text.empty()) {  // every reference caller tests .empty() before it parses
            doc[i] = SBE_JX_EMPTY;
            continue;
        }
        Value root;
        try {
            if (!parse_from_stream(text, root)) {
                doc[i] = SBE_JX_FAILED;
                continue;
            }
        } catch (const std::runtime_error&) {  // "Exceeded stackLimit in readValue()."
            doc[i] = SBE_JX_STACK;
            continue;
        }
        doc[i] = SBE_JX_OK;
        uint32_t o, l;
        describe(root, text, root_kind[i], o, l);
        for (uint32_t p = 0; p < n_paths; ++p) {
            const Value* cur = &root;
            for (const std::string& name : paths[p]) {
                if (!cur->isObject() || !cur->isMember(name)) {
                    cur = nullptr;
                    break;
                }
                cur = &(*cur)[name];
            }
            if (!cur) continue;
            describe(*cur, text, kind[i * n_paths + p], o, l);
            off[i * n_paths + p] = (uint32_t)vo + o;
            len[i * n_paths + p] = l;
        }
    }
}

}  // extern "C"

