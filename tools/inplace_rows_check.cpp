// Stand-alone check of the serving core's in-place request rows (csrc/runtime/serve_core.cpp:
// the row buffer pool, the segment table of a step, the buffers' lifetime) on a CpuDevice, meant
// to be built with the sanitizers (tests/test_inplace_rows.py does):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc/include \
//       -Icsrc/runtime tools/inplace_rows_check.cpp $(ls csrc/runtime/*.cpp | grep -v bindings.cpp) \
//       -o inplace_rows_check -lpthread -lrt && ./inplace_rows_check
// Three cases, each driven from several threads, every answer compared with a second core whose
// device has no in-place mode (response_time_ms removed from both):
//   1. requests of 1 / 37 / 64 / 100 / 129 transactions at step capacity 64, one sender and four
//   2. a step of more than IGP_ROW_SEGS segments, and a step with a unary call in it: packed
//   3. a late step that is held: its failed item returns, its buffer stays out of the pool
// Exit code 0 and "inplace_rows_check: ok": passed.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "cpu_device.h"
#include "cpu_scorer.h"
#include "serve_core.h"

using namespace igp;

namespace {

constexpr int64_t kNow = 1760000000;

[[noreturn]] void die(const std::string& what) {
  std::fprintf(stderr, "inplace_rows_check: FAILED: %s\n", what.c_str());
  std::exit(1);
}
void expect(bool ok, const std::string& what) {
  if (!ok) die(what);
}

// ---- a hand-rolled risk.v1 encoder
void vi(std::string& o, uint64_t v) {
  while (v >= 0x80) {
    o.push_back(char((v & 0x7f) | 0x80));
    v >>= 7;
  }
  o.push_back(char(v));
}
void ld(std::string& o, int field, const std::string& body) {
  vi(o, uint64_t(field) << 3 | 2);
  vi(o, body.size());
  o += body;
}
std::string tx(const std::string& account, int64_t amount, const std::string& type, const std::string& ip,
               const std::string& dev, const std::string& fp) {
  std::string b;
  ld(b, 1, account);
  vi(b, 3 << 3);
  vi(b, uint64_t(amount));
  ld(b, 4, type);
  ld(b, 8, ip);
  ld(b, 9, dev);
  ld(b, 10, fp);
  return b;
}
std::string request(std::mt19937_64& rng, const std::vector<std::string>& ids, size_t n, size_t rot = 0) {
  static const char* types[] = {"deposit", "withdraw", "bet", "win", "bonus", "refund", "chargeback"};
  static const int64_t amounts[] = {1, 127, 128, 500, 150000, 3000000000ll, -5};
  std::string out;
  for (size_t k = 0; k < n; ++k)
    ld(out, 1, tx(ids[(k + rot) % ids.size()], amounts[rng() % 7], types[rng() % 7], "10." + std::to_string(rng() % 250) + ".0.1",
                  "dev-" + std::to_string(rng() % 1000), "fp-" + std::to_string(rng() % 1000)));
  return out;
}
std::vector<std::string> names(const std::string& salt, size_t n) {
  std::vector<std::string> v;
  for (size_t i = 0; i < n; ++i) v.push_back(salt + "-" + std::to_string(i));
  return v;
}

// field 6 (response_time_ms) removed from every entry of a ScoreBatchResponse / from a tx response
uint64_t rd(const std::string& b, size_t& p) {
  uint64_t v = 0;
  for (int s = 0;; s += 7) {
    expect(p < b.size(), "truncated response");
    const uint8_t c = uint8_t(b[p++]);
    v |= uint64_t(c & 0x7f) << s;
    if (!(c & 0x80)) return v;
  }
}
std::string strip_body(const std::string& b) {
  std::string out;
  size_t q = 0;
  while (q < b.size()) {
    const size_t at = q;
    const uint64_t t = rd(b, q);
    const int w = int(t & 7);
    if (w == 0) rd(b, q);
    else if (w == 2) q += rd(b, q);
    else if (w == 5) q += 4;
    else if (w == 1) q += 8;
    else die("wire type in a response");
    expect(q <= b.size(), "field past the end of a response");
    if ((t >> 3) != 6) out.append(b, at, q - at);
  }
  return out;
}
std::string strip_batch(const std::string& b) {
  std::string out;
  size_t p = 0;
  while (p < b.size()) {
    expect(b[p] == 0x0a, "ScoreBatchResponse entry tag");
    ++p;
    const size_t n = rd(b, p);
    expect(p + n <= b.size(), "entry past the end of the response");
    ld(out, 1, strip_body(b.substr(p, n)));
    p += n;
  }
  return out;
}

// ---- one serving stack
struct Stack {
  std::shared_ptr<CpuScorer> sc;
  std::unique_ptr<CpuDevice> dev;
  std::unique_ptr<ServeCore> core;
  Stack(bool inplace, int max_wait_us) {
    sc = std::make_shared<CpuScorer>(8192, 64, 16, 16, 0);
    ScoreCfg c{};
    c.block_threshold = 80;
    c.review_threshold = 50;
    c.max_tx_per_minute = 10;
    c.new_account_days = 7;
    c.large_deposit_amount = 100000;
    c.max_devices_per_day = 3;
    c.max_ips_per_day = 5;
    c.ml_weight = 0.6;
    c.rule_weight = 0.4;
    c.ml_high_risk = 0.7;
    c.ml_error_score = 0.5;
    c.w_high_velocity = 20;
    c.w_new_account_large_tx = 25;
    c.w_multiple_devices = 15;
    c.w_ip_country_mismatch = 10;
    c.w_vpn = 10;
    c.w_rapid_deposit_withdraw = 30;
    c.w_bonus_abuse = 35;
    c.w_known_fraudster = 100;
    c.model_kind = 1;
    c.ml_stride = 1;
    c.session_ttl = 1800;
    c.last_tx_ttl = 86400;
    c.hll_ttl = 86400;
    c.sum_ttl = 3600;
    sc->set_cfg(c);
    dev = std::make_unique<CpuDevice>(sc, 2, 64, inplace);
    ServeCore::Options o;
    o.max_wait_us = max_wait_us;
    o.features = true;
    core = std::make_unique<ServeCore>(std::vector<std::shared_ptr<AccountIndex>>{std::make_shared<AccountIndex>(8192)},
                                       dev->ops(), 0, nullptr, o);
  }
  std::string ask(const std::string& req) { return strip_batch(core->score_batch(req.data(), req.size(), kNow, 0)); }
};

void spin(const std::function<bool()>& cond, const char* what) {
  const auto t_end = std::chrono::steady_clock::now() + std::chrono::seconds(20);
  while (!cond()) {
    if (std::chrono::steady_clock::now() > t_end) die(std::string("timed out: ") + what);
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}

const size_t kSizes[5] = {1, 37, 64, 100, 129};

// case 1. A row's answer depends on which earlier rows of its account sat in earlier steps, so
// accounts repeat within a step only where the cut into steps is fixed (one sender: cut at the
// capacity); the four concurrent senders' accounts appear once per request and again in the
// sender's later requests.
std::vector<std::string> run_streams(Stack& s) {
  std::vector<std::string> got;
  std::mt19937_64 rng(11);
  const auto shared = names("acct", 40);
  for (int k = 0; k < 10; ++k) got.push_back(s.ask(request(rng, shared, kSizes[k < 5 ? k : 9 - k], size_t(k))));
  std::vector<std::vector<std::string>> out(4);
  std::vector<std::thread> th;
  std::atomic<int> ready{0};
  for (int t = 0; t < 4; ++t)
    th.emplace_back([&, t] {
      std::mt19937_64 r(200 + t);
      const auto ids = names("t" + std::to_string(t), 129);
      std::vector<std::string> reqs;
      for (int k = 0; k < 10; ++k) reqs.push_back(request(r, ids, kSizes[(k + t) % 5]));
      ready.fetch_add(1);
      while (ready.load() < 4) std::this_thread::yield();
      for (const auto& q : reqs) out[t].push_back(s.ask(q));
    });
  for (auto& x : th) x.join();
  for (auto& v : out) got.insert(got.end(), v.begin(), v.end());
  return got;
}

void hold_one_step(Stack& s, const std::string& salt) {
  std::mt19937_64 rng(5);
  s.dev->debug_hold_steps(1);
  bool failed = false;
  try {
    s.ask(request(rng, names(salt, 5), 5));
  } catch (const std::exception& e) {
    failed = std::string(e.what()).find("exceeded its deadline") != std::string::npos;
  }
  expect(failed, "the item of a late step did not fail");
  spin([&] { return s.dev->debug_held_steps() == 1; }, "the late step is held");
}

void case_streams() {
  Stack on(true, 200), off(false, 200);
  expect(run_streams(on) == run_streams(off), "answers differ between in-place and packed rows");
  const ServeStats a = on.core->stats(false), b = off.core->stats(false);
  expect(a.inplace_steps > 0 && a.packed_steps == 0 && a.inplace_steps == a.steps, "the on run did not run in place");
  expect(on.dev->gathered_steps() == a.inplace_steps, "the device gathered other steps than the core counted");
  expect(b.inplace_steps == 0 && b.packed_steps == b.steps && b.rowbufs == 0, "the off run ran in place");
  expect(a.rowbufs >= 1 && a.rowbufs == a.rowbufs_free, "a row buffer is missing from the pool");
  on.core->stop();
  expect(on.core->stats(false).rowbufs == 0, "stop() left row buffers allocated");
}

void case_fallback() {
  std::mt19937_64 rng(21);
  std::vector<std::string> small;
  for (int k = 0; k < 20; ++k) small.push_back(request(rng, names("s" + std::to_string(k), 3), size_t(1 + k % 3)));
  const std::string filler = request(rng, names("fill", 64), 64);
  {
    Stack on(true, 60000000), off(false, 200);
    std::vector<std::string> want, got(21);
    for (const auto& q : small) want.push_back(off.ask(q));
    want.push_back(off.ask(filler));
    hold_one_step(on, "held");
    on.core->stats(true);
    std::vector<std::thread> th;
    for (int k = 0; k < 20; ++k) th.emplace_back([&, k] { got[k] = on.ask(small[k]); });
    spin([&] { return on.core->pending_items() == 20; }, "20 small requests queued");
    th.emplace_back([&] { got[20] = on.ask(filler); });
    spin([&] { return on.core->stats(false).steps >= 1; }, "the full step was issued");
    const ServeStats st = on.core->stats(false);
    expect(st.packed_steps == 1 && st.inplace_steps == 0 && st.max_step_rows == 64, "a step of 21 segments was not packed");
    on.dev->debug_release_steps();
    for (auto& x : th) x.join();
    expect(got == want, "answers of the packed step differ");
    expect(on.core->stats(false).inplace_steps >= 1, "the filler's other rows did not run in place");
  }
  {  // a unary call and a batch item in one step
    Stack on(true, 60000000), off(false, 200);
    const std::string one = tx("unary-acct", 700, "deposit", "10.0.0.1", "dev-1", "fp-1");
    const std::string req = request(rng, names("mixed", 64), 64);
    std::vector<ServeCore::Done> dw, dg;
    off.core->submit_tx(one.data(), one.size(), 7, kNow, 0);
    spin([&] { return off.core->poll(dw, 1, 1000) + dw.size() > 0; }, "unary answer (packed core)");
    const std::string want = off.ask(req);
    hold_one_step(on, "held");
    on.core->stats(true);
    on.core->submit_tx(one.data(), one.size(), 7, kNow, 0);
    std::string got;
    std::thread t([&] { got = on.ask(req); });
    spin([&] { return on.core->stats(false).steps >= 1; }, "the mixed step was issued");
    const ServeStats st = on.core->stats(false);
    expect(st.packed_steps == 1 && st.inplace_steps == 0 && st.unary == 1 && st.max_step_rows == 64,
           "a step with a unary call was not packed");
    on.dev->debug_release_steps();
    t.join();
    spin([&] { return on.core->poll(dg, 1, 1000) + dg.size() > 0; }, "unary answer");
    expect(dg[0].err.empty() && dw[0].err.empty() && dg[0].tag == 7, "unary call failed");
    expect(strip_body(dg[0].bytes) == strip_body(dw[0].bytes), "unary answers differ");
    expect(got == want, "batch answers of the mixed step differ");
  }
}

void case_lifetime() {
  std::mt19937_64 rng(23);
  const std::string later = request(rng, names("later", 37), 37);
  Stack on(true, 200), off(false, 200);
  const std::string want_later = off.ask(later);
  hold_one_step(on, "held");
  ServeStats st = on.core->stats(false);
  expect(st.rowbufs == 1 && st.rowbufs_free == 0, "the held step's buffer went back to the pool");
  std::string got;
  std::thread t([&] { got = on.ask(later); });
  spin([&] { return on.core->stats(false).rowbufs == 2; }, "the later request took a buffer of its own");
  expect(on.core->stats(false).rowbufs_free == 0, "a buffer is free while both are in use");
  on.dev->debug_release_steps();
  t.join();
  expect(got == want_later, "the later request's answer differs");
  spin([&] { return on.core->stats(false).rowbufs_free == 2; }, "both buffers back after the release");
  for (size_t n : {size_t(1), size_t(100), size_t(129)}) {
    const std::string q = request(rng, names("after" + std::to_string(n), n), n);
    expect(on.ask(q) == off.ask(q), "a request after the held step is answered differently");
  }
  on.dev->debug_fail_steps(1, 0);
  bool failed = false;
  try {
    on.ask(request(rng, names("failed", 37), 37));
  } catch (const std::exception& e) {
    failed = std::string(e.what()).find("injected step failure") != std::string::npos;
  }
  expect(failed, "the injected failure did not fail the item");
  spin([&] { const ServeStats s = on.core->stats(false); return s.rowbufs == s.rowbufs_free; }, "a failed step leaked a buffer");
  const std::string again = request(rng, names("again", 65), 65);
  expect(on.ask(again) == off.ask(again), "the request after a failed step is answered differently");
  on.core->stop();
  st = on.core->stats(false);
  expect(st.rowbufs == 0 && st.rowbufs_free == 0, "stop() left row buffers allocated");
}

}  // namespace

int main() {
  case_streams();
  case_fallback();
  case_lifetime();
  std::printf("inplace_rows_check: ok\n");
  return 0;
}
