// Upper bound on how many rows of one scoring step belong to the same account, from a small
// counting sketch over the rows' feature-store slots. The device's K1 scores and applies every
// account with at most IGP_K1_SEG_MAX events in a batch by itself (csrc/kernels/launch.h
// K1_SEG_MAX); the multi-event update launch behind it is needed only when some account has
// more. The sketch proves the common case cheaply and exactly in one direction: the bound is
// never below the true maximum multiplicity, so "bound <= IGP_K1_SEG_MAX" means the update
// launch would find nothing to do.
//
// One counter per hash bucket of the slot; the largest counter bounds every account's count
// (rows of one account share a bucket; other accounts in it only add). The bound is reported
// saturated at kMultUnknown (255, "no bound"): a caller only asks whether it is at most
// IGP_K1_SEG_MAX. Rows with slot < 0 (unknown account) are applied by no one and are not
// counted. Plain C++, shared by the host runtime (per request, on the ingress threads) and the
// native pipeline driver (which builds it in the same pass that copies the rows into its slab).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "records.h"

namespace igp {

constexpr int IGP_K1_SEG_MAX = 16;           // == K1_SEG_MAX (static_assert in csrc/kernels/driver.hip)
constexpr int kMultSketchBits = 13;          // 8192 counters: 8192 uniform rows stay far below the bound
constexpr int kMultSketchSize = 1 << kMultSketchBits;
constexpr int kMultUnknown = 255;            // "no bound": where the reported bound saturates
constexpr int kMultCombineMax = 4;           // items whose counters a step adds up (more: sum of maxima only)

inline uint32_t mult_sketch_index(int32_t slot) {
  return (uint32_t(slot) * 0x9E3779B1u) >> (32 - kMultSketchBits);
}

// The sketch of one item (a request's rows): `max` alone for an item that needs no counters
// (0 or 1 counted rows), else the counters too. max == kMultUnknown: no bound is known.
// Counters are 16 bits wide and cannot wrap (items of 65535 rows or more claim no bound), so
// the counting loop is branch-free: one add per row, the maximum taken afterwards in one
// vectorisable scan of the 16 KB table.
struct MultSketch {
  std::vector<uint16_t> c;  // empty, or kMultSketchSize counters
  int max = kMultUnknown;

  // `dst` (nullable): the rows are also copied there, in the same pass over them
  void build(const ReqRec* rows, size_t n, ReqRec* dst = nullptr) {
    max = 0;
    if (n <= 1 || n >= 65535) {
      c.clear();
      if (dst && n) std::memcpy(dst, rows, n * sizeof(ReqRec));
      max = n == 0 ? 0 : n == 1 ? (rows[0].slot >= 0 ? 1 : 0) : kMultUnknown;
      return;
    }
    c.assign(size_t(kMultSketchSize), 0);
    uint16_t* const cnt = c.data();
    if (dst) {
      for (size_t k = 0; k < n; ++k) {
        const int32_t slot = rows[k].slot;
        std::memcpy(dst + k, rows + k, sizeof(ReqRec));
        cnt[mult_sketch_index(slot)] += uint16_t(slot >= 0);
      }
    } else {
      for (size_t k = 0; k < n; ++k) {
        const int32_t slot = rows[k].slot;
        cnt[mult_sketch_index(slot)] += uint16_t(slot >= 0);
      }
    }
    uint16_t m = 0;
    for (int b = 0; b < kMultSketchSize; ++b) m = std::max(m, cnt[b]);
    max = std::min(int(m), kMultUnknown);
  }
};

// Bound for a step made of (parts of) `n` items; a part of an item is bounded by the whole item.
//  * one item: its own maximum, O(1) - a full batch per request, the serving benchmark's case;
//  * the sum of the items' maxima bounds any account's count across them: enough for steps of
//    a few requests, and O(n);
//  * otherwise, up to kMultCombineMax items with counters are added bucket by bucket; beyond
//    that no bound below the sum is claimed and the caller launches the update.
// `scratch` is caller-owned working memory (kMultSketchSize words once used).
inline int mult_step_bound(const MultSketch* const* items, size_t n, std::vector<uint32_t>& scratch) {
  if (n == 0) return 0;
  int sum = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!items[i] || items[i]->max >= kMultUnknown) return kMultUnknown;
    sum += items[i]->max;
    if (sum >= kMultUnknown) sum = kMultUnknown;
  }
  if (n == 1 || sum <= IGP_K1_SEG_MAX) return sum;
  if (n > size_t(kMultCombineMax)) return sum;
  scratch.assign(size_t(kMultSketchSize), 0);
  int rest = 0;  // items without counters (at most one counted row each) land in unknown buckets
  for (size_t i = 0; i < n; ++i) {
    const MultSketch& s = *items[i];
    if (s.c.size() != size_t(kMultSketchSize)) {
      rest += s.max;
      continue;
    }
    for (int b = 0; b < kMultSketchSize; ++b) scratch[size_t(b)] += s.c[size_t(b)];
  }
  uint32_t m = 0;
  for (int b = 0; b < kMultSketchSize; ++b) m = std::max(m, scratch[size_t(b)]);
  return int(std::min<uint32_t>(m + uint32_t(rest), uint32_t(kMultUnknown)));
}

}  // namespace igp
