// Membership test of a BRANCH_MEMBER (mode 6) tree node against the ensemble's set table
// (layout: csrc/runtime/trees.h). The table is small, read from global memory and stays in L2.
// The host validates every offset and length before upload (models/plan.py); the range guards
// here only keep a table that skipped that check from turning into an out-of-range read.
#pragma once
#include "common.h"

namespace igp {

constexpr uint32_t TSET_LIST = 0x80000000u;  // header: kind << 31 | length
constexpr uint32_t TSET_CAP = 256;           // bitsets hold the integers [0, TSET_CAP)
constexpr int TSET_STEPS = 31;               // bisection trip bound: list lengths are < 2^31

__device__ __forceinline__ bool tree_set_member(const uint32_t* __restrict__ sets, uint32_t n_words,
                                                uint32_t off, float x) {
  if (off >= n_words) return false;
  // range and integrality first, so the conversion is always defined (1e30, inf, -1, 2.5 and NaN
  // all stop here). The bitset word x would select is loaded beside the header, not after it -
  // one round trip decides a bitset - with its index held inside the table for the sets (short
  // bitsets, lists) where that word is not the set's
  const bool intx = x >= 0.f && x < (float)TSET_CAP && x == truncf(x);
  const uint32_t v = intx ? (uint32_t)x : 0u;
  const uint32_t wi = off + 1 + (v >> 5);
  const uint32_t h = sets[off];
  const uint32_t w = sets[wi < n_words ? wi : n_words - 1];
  const uint32_t len = h & ~TSET_LIST;
  if (len > n_words - off - 1) return false;
  if (!(h & TSET_LIST)) return intx && (v >> 5) < len && ((w >> (v & 31u)) & 1u);
  const uint32_t* d = sets + off + 1;
  // sorted distinct floats: lower bound, then one equality (NaN compares false everywhere)
  uint32_t lo = 0, n = len;
  for (int it = 0; it < TSET_STEPS && n > 0; ++it) {
    const uint32_t half = n >> 1;
    const float m = __uint_as_float(d[lo + half]);
    if (m < x) {
      lo += half + 1;
      n -= half + 1;
    } else {
      n = half;
    }
  }
  return lo < len && __uint_as_float(d[lo]) == x;
}

}  // namespace igp
