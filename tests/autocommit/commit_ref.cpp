// TEST ONLY: an independent restatement of the reference's auto-commit decision, for the tests of
// sbe_classify_commits.  Where the device code walks a document as a stream of tokens, this one
// builds a tree (a recursive reader with the semantics of jsoncpp 1.9.5's OurReader under
// CharReaderBuilder defaults, function by function) and then asks the tree the questions the
// reference asks of its Json::Value: extract_topic_from_message (src/cluster_client.cpp:756-806),
// should_skip_auto_commit (:847-886) and the commit branch of handle_incoming_message (:1251),
// in the reference's structure.  jsoncpp itself is not available to the tests: the reader is
// pinned to the project's oracle instead (cref_seq computes ParseResult.sequence_number,
// src/sbe_encoder.cpp:1031-1125, on the same tree; a CPU test compares it with orc_seq_eval).
#include <cmath>
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
    size_t tok_s = 0, tok_e = 0;  // the token in the document (strings: with the quotes)

    bool isMember(const char* key) const {  // JSON_ASSERT_MESSAGE: null or object, else throws
        if (type == Null) return false;
        if (type != Object) throw std::logic_error("isMember: not an object");
        return obj.count(key) != 0;
    }
    const Value& operator[](const char* key) const {
        static const Value null_value;
        if (type == Null) return null_value;
        if (type != Object) throw std::logic_error("operator[]: not an object");
        auto it = obj.find(key);
        return it == obj.end() ? null_value : it->second;
    }
    bool isObject() const { return type == Object; }
    // asString: only the string kinds' text is ever compared; numbers keep their token text here
    // (jsoncpp prints them as decimal / %.17g), which can equal neither a control topic nor, by
    // the interface's rule, a table entry (SBE_TOPIC_HOST)
    std::string asString(const std::string& doc) const {
        switch (type) {
            case Null: return "";
            case String: return s;
            case Bool: return b ? "true" : "false";
            case Int: case UInt: case Real: return doc.substr(tok_s, tok_e - tok_s);
            default: throw std::logic_error("Type is not convertible to string");
        }
    }
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
            case ObjectBegin: return readObject(v);
            case ArrayBegin: return readArray(v);
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

// ---- ParseResult.sequence_number on the tree (src/sbe_encoder.cpp:1031-1125) ----
uint64_t x86_cast_u64(double d) {  // static_cast<uint64_t>(double) as x86-64 gcc compiles it
    if (d != d) return 0x8000000000000000ull;
    if (d >= 18446744073709551616.0) return 0;
    if (d >= 9223372036854775808.0) return (uint64_t)d;
    if (d < -9223372036854775808.0) return 0x8000000000000000ull;
    return (uint64_t)(int64_t)d;
}
bool integral(double d) {
    double ip;
    return std::modf(d, &ip) == 0.0;
}
uint64_t extract_sequence(const Value& obj) {
    if (!obj.isObject()) return 0;
    if (!obj.isMember("_sequence_number")) return 0;
    const Value& v = obj["_sequence_number"];
    switch (v.type) {
        case Value::Int: return (uint64_t)v.i;  // isUInt64 (>= 0) or isInt64
        case Value::UInt: return v.u;
        case Value::Real:
            if (v.d >= 0 && v.d < 18446744073709551616.0 && integral(v.d)) return (uint64_t)v.d;        // isUInt64
            if (v.d >= -9223372036854775808.0 && v.d < 9223372036854775808.0 && integral(v.d))          // isInt64
                return (uint64_t)(int64_t)v.d;
            return x86_cast_u64(v.d);  // isNumeric
        case Value::String: {           // std::stoull(asString()) over c_str(); exceptions give 0
            const char* s = v.s.c_str();
            size_t i = 0;
            while (s[i] == ' ' || (s[i] >= 9 && s[i] <= 13)) ++i;
            bool neg = false;
            if (s[i] == '+' || s[i] == '-') neg = s[i++] == '-';
            if (s[i] < '0' || s[i] > '9') return 0;
            uint64_t r = 0;
            for (; s[i] >= '0' && s[i] <= '9'; ++i) {
                const uint64_t dg = s[i] - '0';
                if (r > (~0ull - dg) / 10) return 0;
                r = r * 10 + dg;
            }
            return neg ? 0 - r : r;
        }
        default: return 0;  // bool, null, containers: none of the four tests holds
    }
}

uint64_t sequence_number(const std::string& payload) {
    uint64_t result = 0;
    try {
        if (payload.empty()) return 0;
        Value root;
        if (!parse_from_stream(payload, root)) return 0;
        if (root.isMember("_sequence_number")) {
            const uint64_t s = extract_sequence(root);
            if (s > 0) result = s;
        }
        if (result == 0 && root.isMember("message") && root["message"].isObject()) {
            const uint64_t s = extract_sequence(root["message"]);
            if (s > 0) result = s;
        }
        if (result == 0 && root.isMember("message") && root["message"].isObject()) {
            const Value& m = root["message"];
            if (m.isMember("message") && m["message"].isObject()) {
                const uint64_t s = extract_sequence(m["message"]);
                if (s > 0) result = s;
            }
        }
        if (result == 0 && root.isMember("message") && root["message"].isObject()) {
            const Value& m = root["message"];
            if (m.isMember("message") && m["message"].isObject()) {
                const Value& mm = m["message"];
                if (mm.isMember("message") && mm["message"].isObject()) {
                    const uint64_t s = extract_sequence(mm["message"]);
                    if (s > 0) result = s;
                }
            }
        }
    } catch (const std::exception&) {
        result = 0;
    }
    return result;
}

// ---- the three reference functions ----
struct ParseResult {
    bool success = false;
    std::string message_type, message_id, payload, headers;
};
struct Topic {
    std::string text;
    uint32_t src = SBE_TOPIC_SRC_FALLBACK, kind = SBE_TOPIC_KIND_NONE;
    size_t s = 0, e = 0;  // token range inside its source string
};

Topic topic_of(const Value& v, const std::string& doc, uint32_t src) {
    Topic t;
    t.text = v.asString(doc);  // throws for arrays and objects
    t.src = src;
    t.s = v.tok_s;
    t.e = v.tok_e;
    switch (v.type) {
        case Value::String:
            ++t.s;
            --t.e;
            t.kind = doc.find('\\', t.s) < t.e ? SBE_TOPIC_KIND_STRING_ESC : SBE_TOPIC_KIND_STRING;
            break;
        case Value::Bool: t.kind = v.b ? SBE_TOPIC_KIND_TRUE : SBE_TOPIC_KIND_FALSE; break;
        case Value::Null: t.kind = SBE_TOPIC_KIND_NULL; break;
        default: t.kind = SBE_TOPIC_KIND_NUMBER; break;
    }
    return t;
}

Topic extract_topic_from_message(const ParseResult& result, const std::string& fallback) {
    if (!result.headers.empty()) {
        try {
            Value root;
            if (parse_from_stream(result.headers, root)) {
                if (root.isMember("topic")) return topic_of(root["topic"], result.headers, SBE_TOPIC_SRC_HEADERS);
            }
        } catch (const std::exception&) {
        }
    }
    if (!result.payload.empty()) {
        try {
            Value root;
            if (parse_from_stream(result.payload, root)) {
                if (root.isMember("topic")) return topic_of(root["topic"], result.payload, SBE_TOPIC_SRC_PAYLOAD);
                if (root.isMember("message") && root["message"].isMember("topic"))
                    return topic_of(root["message"]["topic"], result.payload, SBE_TOPIC_SRC_PAYLOAD_MESSAGE);
            }
        } catch (const std::exception&) {
        }
    }
    Topic t;
    t.text = fallback;  // *subscribed_topics_.begin(), or "default": the caller's
    return t;
}

// should_skip_auto_commit, returning which clause fired (0: not skipped)
uint32_t should_skip_auto_commit(const ParseResult& result, const std::string& fallback, Topic& topic, bool& extracted) {
    extracted = false;
    if (result.message_type == "acknowledgment" || result.message_type == "acknowledgment_legacy" ||
        result.message_type == "Acknowledgment" || result.message_type == "Acknowledgment_legacy" ||
        result.message_type == "COMMIT_RESPONSE" || result.message_type == "SUBSCRIBE")
        return SBE_CM_SKIP_TYPE;
    if (!result.message_id.empty() && result.message_id.find("ack_") == 0) return SBE_CM_SKIP_ACK_ID;
    topic = extract_topic_from_message(result, fallback);
    extracted = true;
    if (topic.text == "_ack" || topic.text == "_subscriptions") return SBE_CM_SKIP_TOPIC;
    if (topic.text == "_control") {
        if (result.message_type == "REPLAY_COMPLETE" || result.payload.find("REPLAY_COMPLETE") != std::string::npos)
            return 0;
        return SBE_CM_SKIP_CONTROL;
    }
    if (result.payload.empty()) return SBE_CM_SKIP_EMPTY_PAYLOAD;
    return 0;
}

}  // namespace

extern "C" {

uint64_t cref_seq(const uint8_t* p, uint64_t n) {
    return sequence_number(std::string(reinterpret_cast<const char*>(p), n));
}

// The arguments of sbe_classify_commits, in host memory.
void cref_classify(const uint8_t* in, const uint64_t* rec_off, uint64_t n, const uint8_t* status, const uint8_t* flags,
                   const uint32_t* view_off, const uint32_t* view_len, const uint8_t* tarena, const uint32_t* toff,
                   uint32_t k, uint8_t* cm, uint8_t* src, uint8_t* kind, uint32_t* off, uint32_t* len, uint32_t* idx,
                   uint64_t* last, uint64_t* count) {
    std::vector<std::string> table;
    for (uint32_t j = 0; j < k; ++j) {
        const uint32_t a = toff[j] < SBE_COMMIT_TABLE_BYTES ? toff[j] : SBE_COMMIT_TABLE_BYTES;
        const uint32_t b = toff[j + 1] < SBE_COMMIT_TABLE_BYTES ? toff[j + 1] : SBE_COMMIT_TABLE_BYTES;
        table.emplace_back(reinterpret_cast<const char*>(tarena) + a, b > a ? b - a : 0);
    }
    for (uint32_t j = 0; j < k; ++j) last[j] = ~0ull;
    for (uint32_t j = 0; j < k + 2; ++j) count[j] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        cm[i] = SBE_CM_NOT_PARSED;
        src[i] = SBE_TOPIC_SRC_NONE;
        kind[i] = SBE_TOPIC_KIND_NONE;
        off[i] = len[i] = 0;
        idx[i] = SBE_TOPIC_UNKNOWN;
        if (status[i] >= 16) continue;
        if (status[i] == SBE_ST_SESSION_EVENT) {  // message_id is never set: no commit, whatever should_skip says
            cm[i] = SBE_CM_NO_ID;
            continue;
        }
        ParseResult r;
        r.success = true;
        const char* rec = reinterpret_cast<const char*>(in) + rec_off[i];
        auto view = [&](int v) { return std::string(rec + view_off[5 * i + v], view_len[5 * i + v]); };
        if (status[i] == SBE_ST_ACK) {
            r.message_type = "Acknowledgment";  // src/sbe_encoder.cpp:921
        } else {
            r.message_type = view(1);
            r.message_id = view(2);
            r.payload = view(3);
            if (!(flags[i] & SBE_FL_HEADERS_E100)) r.headers = view(4);
        }
        Topic t;
        bool extracted;
        const uint32_t skip = should_skip_auto_commit(r, table[0], t, extracted);
        if (extracted) {
            src[i] = (uint8_t)t.src;
            kind[i] = (uint8_t)t.kind;
            if (t.src != SBE_TOPIC_SRC_FALLBACK) {
                off[i] = (uint32_t)(view_off[5 * i + (t.src == SBE_TOPIC_SRC_HEADERS ? 4 : 3)] + t.s);
                len[i] = (uint32_t)(t.e - t.s);
            }
        }
        if (skip) {
            cm[i] = (uint8_t)skip;
            continue;
        }
        if (r.message_id.empty()) {  // :1251
            cm[i] = SBE_CM_NO_ID;
            continue;
        }
        cm[i] = SBE_CM_COMMIT;
        uint32_t slot;
        if (t.src == SBE_TOPIC_SRC_FALLBACK) {
            idx[i] = 0;
        } else if (t.kind != SBE_TOPIC_KIND_STRING && t.kind != SBE_TOPIC_KIND_STRING_ESC) {
            idx[i] = SBE_TOPIC_HOST;
        } else {
            for (uint32_t j = 0; j < k; ++j)
                if (table[j] == t.text) {
                    idx[i] = j;
                    break;
                }
        }
        slot = idx[i] == SBE_TOPIC_UNKNOWN ? k : idx[i] == SBE_TOPIC_HOST ? k + 1 : idx[i];
        ++count[slot];
        if (slot < k) last[slot] = i;
    }
}

}  // extern "C"
