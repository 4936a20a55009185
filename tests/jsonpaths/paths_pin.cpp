// TEST ONLY: the older copy of the tree-building reader (tests/autocommit/commit_ref.cpp, which a
// CPU test pins to the oracle's orc_seq_eval) with the canonical dump of tree_dump.hpp behind it,
// so that a CPU test can hold the newer copy in paths_ref.cpp to it: the same verdict and the same
// dump on every document.
#include <cstdio>

#include "../autocommit/commit_ref.cpp"

namespace {
#include "tree_dump.hpp"
}  // namespace

extern "C" uint64_t cpin_dump(const uint8_t* p, uint64_t n, uint32_t* verdict, char* out, uint64_t cap) {
    return dump_document<Value>(std::string(reinterpret_cast<const char*>(p), n), verdict, out, cap);
}
