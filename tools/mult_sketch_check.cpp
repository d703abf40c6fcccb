// Stand-alone check of csrc/include/mult_sketch.h (the bound that lets the native driver skip the
// multi-event update launch), meant to be built with the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Icsrc/include tools/mult_sketch_check.cpp -o /tmp/mult_sketch_check && /tmp/mult_sketch_check
// Random steps, split into random items, sketched per item and combined as the serving core's
// stepper does; the bound must never be below the true maximum multiplicity. Exit code 0: ok.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>

#include "mult_sketch.h"

using namespace igp;

static int true_max(const std::vector<ReqRec>& rows) {
  std::map<int32_t, int> cnt;
  int m = 0;
  for (const ReqRec& r : rows)
    if (r.slot >= 0) m = std::max(m, ++cnt[r.slot]);
  return m;
}

static int step_bound(const std::vector<ReqRec>& rows, const std::vector<size_t>& sizes) {
  std::vector<MultSketch> items(sizes.size());
  size_t at = 0;
  for (size_t i = 0; i < sizes.size(); ++i) {
    items[i].build(rows.data() + at, sizes[i]);
    at += sizes[i];
  }
  std::vector<const MultSketch*> parts;
  for (const MultSketch& s : items) parts.push_back(&s);
  std::vector<uint32_t> scratch;
  return mult_step_bound(parts.data(), parts.size(), scratch);
}

static int fail(const char* what, int bound, int truth) {
  std::fprintf(stderr, "mult_sketch_check: %s: bound %d, true maximum %d\n", what, bound, truth);
  return 1;
}

int main() {
  std::mt19937_64 rng(12345);
  int checked = 0;
  for (int round = 0; round < 400; ++round) {
    const size_t n = size_t(rng() % 9000);
    const int64_t space = int64_t(1) << (1 + rng() % 21);
    std::vector<ReqRec> rows(n);
    for (ReqRec& r : rows) r.slot = int32_t(int64_t(rng() % uint64_t(space + 1)) - 1);  // -1: unknown account
    if (n > 0 && round % 7 == 0) {  // one heavy account, up to and past the counters' saturation
      const size_t k = size_t(rng() % 400) % n;
      for (size_t i = 0; i < k; ++i) rows[size_t(rng() % n)].slot = 4242;
    }
    std::vector<size_t> sizes;
    size_t left = n;
    const int pieces = 1 + int(rng() % 8);
    for (int p = 0; p + 1 < pieces && left > 0; ++p) {
      const size_t take = size_t(rng() % (left + 1));
      sizes.push_back(take);
      left -= take;
    }
    sizes.push_back(left);
    const int truth = std::min(true_max(rows), kMultUnknown);
    const int b = step_bound(rows, sizes);
    if (b < truth) return fail("split step", b, truth);
    const int whole = step_bound(rows, {n});
    if (whole < truth) return fail("one item", whole, truth);
    // the copying form (the pipeline driver's row copy): same bound, rows copied exactly
    std::vector<ReqRec> dst(n);
    MultSketch cp;
    cp.build(rows.data(), n, dst.data());
    if (cp.max != whole) return fail("copying build differs", cp.max, whole);
    if (n && std::memcmp(dst.data(), rows.data(), n * sizeof(ReqRec)) != 0) return fail("copy", 0, 0);
    ++checked;
  }
  {  // 8192 uniform rows over 2^20 accounts: the benchmark's shape must stay skippable
    for (int round = 0; round < 20; ++round) {
      std::vector<ReqRec> rows(8192);
      for (ReqRec& r : rows) r.slot = int32_t(rng() % (1u << 20));
      const int b = step_bound(rows, {rows.size()});
      if (b < true_max(rows)) return fail("uniform", b, true_max(rows));
      if (b > IGP_K1_SEG_MAX) return fail("uniform 8192 / 2^20 above K1_SEG_MAX", b, true_max(rows));
      ++checked;
    }
  }
  {  // exactly K1_SEG_MAX and one more
    for (int k : {IGP_K1_SEG_MAX, IGP_K1_SEG_MAX + 1, 300}) {
      std::vector<ReqRec> rows(size_t(k) + 100);
      for (size_t i = 0; i < rows.size(); ++i) rows[i].slot = i < size_t(k) ? 99 : int32_t(100000 + 37 * i);
      const int b = step_bound(rows, {rows.size()});
      if (b < std::min(k, kMultUnknown)) return fail("heavy account", b, k);
      ++checked;
    }
  }
  std::printf("mult_sketch_check: %d steps ok\n", checked);
  return 0;
}
