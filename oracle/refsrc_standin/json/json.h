// json/json.h — TEST INFRASTRUCTURE ONLY: a stand-in for the part of jsoncpp's interface that the
// reference's MessageParser uses for ParseResult.sequence_number (src/sbe_encoder.cpp:1035-1125),
// so that file can be compiled where it lies into oracle/_ref/libsbe_ref_src.so.  jsoncpp itself
// is not available to the tests.
//
// The reader underneath is the project's own tree reader (tests/autocommit/commit_ref.cpp: a
// restatement of jsoncpp 1.9.5's OurReader under CharReaderBuilder defaults, which a CPU test pins
// to orc_seq_eval), included, not copied.  The is* / as* accessors below follow jsoncpp 1.9.5's
// json_value.cpp.  What this makes checkable is the reference's own lookup (four locations,
// `seq > 0` fall-through, conversion order, stoull, catch); the reader stays ours and unpinned.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <istream>
#include <iterator>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/sbecodec.h"

namespace refsrc_standin {
#include "../../../tests/autocommit/commit_ref.cpp"
}  // namespace refsrc_standin

namespace Json {

using Int64 = std::int64_t;
using UInt64 = std::uint64_t;
using String = std::string;

class LogicError : public std::logic_error {  // what JSON_ASSERT / JSON_FAIL_MESSAGE throw
public:
    using std::logic_error::logic_error;
};

class Value {
    using Tree = refsrc_standin::Value;
    Tree v_;

    static bool integral(double d) {  // IsIntegral
        double ip;
        return std::modf(d, &ip) == 0.0;
    }
    static constexpr double kMaxUInt64AsDouble = 18446744073709551615.0;  // rounds to 2^64
    static bool in_range(double d, double lo, double hi) { return d >= lo && d <= hi; }  // InRange

public:
    Value() = default;
    explicit Value(const Tree& t) : v_(t) {}
    Tree& tree() { return v_; }

    bool isObject() const { return v_.type == Tree::Object; }
    bool isString() const { return v_.type == Tree::String; }
    bool isMember(const char* key) const { return v_.isMember(key); }
    bool isMember(const String& key) const { return v_.isMember(key.c_str()); }
    // const and non-const alike hand out a copy: the caller never assigns through operator[]
    Value operator[](const char* key) const { return Value(v_[key]); }
    Value operator[](const String& key) const { return Value(v_[key.c_str()]); }

    bool isUInt64() const {
        switch (v_.type) {
            case Tree::Int: return v_.i >= 0;
            case Tree::UInt: return true;
            case Tree::Real: return v_.d >= 0 && v_.d < kMaxUInt64AsDouble && integral(v_.d);
            default: return false;
        }
    }
    bool isInt64() const {
        switch (v_.type) {
            case Tree::Int: return true;
            case Tree::UInt: return v_.u <= (UInt64)INT64_MAX;
            case Tree::Real:
                return v_.d >= double(INT64_MIN) && v_.d < double(INT64_MAX) && integral(v_.d);
            default: return false;
        }
    }
    bool isNumeric() const { return v_.type == Tree::Int || v_.type == Tree::UInt || v_.type == Tree::Real; }

    UInt64 asUInt64() const {
        switch (v_.type) {
            case Tree::Int:
                if (v_.i < 0) throw LogicError("LargestInt out of UInt64 range");
                return (UInt64)v_.i;
            case Tree::UInt: return v_.u;
            case Tree::Real:
                if (!in_range(v_.d, 0, kMaxUInt64AsDouble)) throw LogicError("double out of UInt64 range");
                return (UInt64)v_.d;
            case Tree::Null: return 0;
            case Tree::Bool: return v_.b ? 1 : 0;
            default: throw LogicError("Value is not convertible to UInt64.");
        }
    }
    Int64 asInt64() const {
        switch (v_.type) {
            case Tree::Int: return v_.i;
            case Tree::UInt:
                if (!isInt64()) throw LogicError("LargestUInt out of Int64 range");
                return (Int64)v_.u;
            case Tree::Real:
                if (!in_range(v_.d, double(INT64_MIN), double(INT64_MAX))) throw LogicError("double out of Int64 range");
                return (Int64)v_.d;
            case Tree::Null: return 0;
            case Tree::Bool: return v_.b ? 1 : 0;
            default: throw LogicError("Value is not convertible to Int64.");
        }
    }
    double asDouble() const {
        switch (v_.type) {
            case Tree::Int: return (double)v_.i;
            case Tree::UInt: return (double)v_.u;
            case Tree::Real: return v_.d;
            case Tree::Null: return 0.0;
            case Tree::Bool: return v_.b ? 1.0 : 0.0;
            default: throw LogicError("Value is not convertible to double.");
        }
    }
    // only a string's text is asked for by the caller (isString() guards it); the number and
    // bool forms are jsoncpp's for completeness of the switch
    String asString() const {
        switch (v_.type) {
            case Tree::Null: return "";
            case Tree::String: return v_.s;
            case Tree::Bool: return v_.b ? "true" : "false";
            case Tree::Int: return std::to_string((long long)v_.i);
            case Tree::UInt: return std::to_string((unsigned long long)v_.u);
            default: throw LogicError("Type is not convertible to string");
        }
    }
};

class CharReaderBuilder {};  // the defaults are the only settings the caller uses

// The whole stream is the document (jsoncpp copies sin.rdbuf()); false on a parse error.  The
// reader's stack-limit exception propagates, as jsoncpp's does.
inline bool parseFromStream(const CharReaderBuilder&, std::istream& sin, Value* root, String* errs) {
    const String doc((std::istreambuf_iterator<char>(sin)), std::istreambuf_iterator<char>());
    const bool ok = refsrc_standin::parse_from_stream(doc, root->tree());
    if (!ok && errs) *errs = "parse error";
    return ok;
}

}  // namespace Json
