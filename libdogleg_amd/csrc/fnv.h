// fnv.h -- 64-bit FNV-1a over integers (every value enters as the 8 bytes of its int64), for the hashes that pin a
// schedule bit for bit: sparse_region.cpp (region_plan_hash, fac_levels_hash), sparse_symbolic_hash.cpp (sym_hash).
#pragma once
#include <cstdint>

struct Fnv
{
  uint64_t h = 1469598103934665603ull;
  template <class... T> void add(T... x)
  { for(int64_t v : {(int64_t)x...}) for(int k = 0; k < 8; k++) { h ^= ((uint64_t)v >> (8*k)) & 0xff; h *= 1099511628211ull; } }
};
