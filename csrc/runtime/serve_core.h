// Native serving core: the risk.v1 scoring hot path from request bytes to response bytes,
// GIL-free, one per GPU (or CPU) shard.
//
//   caller threads (gRPC handlers, bench ingress threads)
//     ScoreBatch bytes -> wire parse (AoS rows, digests) -> AccountIndex resolve (node-shared
//     in multi-rank serving) -> owner sort -> enqueue one work item, wait for its rows
//   stepper thread
//     forms device micro-batches from the FIFO of items (up to the pipeline's capacity, or
//     per-owner chunk capacity in exchange mode), packs the rows into the slot's pinned
//     buffer, launches the slot through the device function table (device_ops.h).
//     A direct device that offers it (device_ops.h host_alloc / row_segs) reads ScoreBatch rows
//     in place: the ingress thread resolves them into a pinned buffer from the core's pool, and
//     the stepper only writes the slot's segment table. A step holds a reference on every
//     buffer it names until it is released, so a late or failed step never reads rows of a
//     later request. Steps with unary calls, score_rows items or more than IGP_ROW_SEGS
//     segments are packed
//   completion thread
//     waits for slots in submit order; unary items are finished (copy + serialise) by a
//     finisher pool and handed back through a completion queue polled from Python
//   callers
//     ScoreBatch on a direct (non-exchange) device: each segment of the request is serialised
//     straight from the slot's pinned result / feature buffers into the response buffer, in row
//     order, and the slot is released after that (no staging copy). A row's response_time_ms is
//     therefore the time from the call's t0 to the serialisation of ITS segment: for a request
//     of one segment that is what it always was, less the serialisation itself; the segments of
//     a longer request carry the time each of them was answered. Exchange devices and
//     score_rows copy their (owner-permuted) rows out first and serialise afterwards, all rows
//     stamped at the end
//
// Unary ScoreTransaction calls are ordinary 1-row items in the same FIFO, so concurrent
// unary calls and batches share device micro-batches (the MPSC micro-batcher of SURVEY 3.6b).
//
// Multi-rank exchange (one process per GPU, every rank ingests): a step on one rank is a
// collective over all ranks, so every rank must issue the same sequence of steps. Ranks share
// a StepClock in /dev/shm: each posts its issued-step count, a rank with nothing queued issues
// an empty step as soon as a peer is ahead of it (and only then: an idle node issues nothing),
// and stop / pause converge every rank to the same count. No host collective, no lock and no
// per-step header on the hot path (VERDICT r2 "step clock").
#pragma once
#include <atomic>
#include <functional>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../include/device_ops.h"
#include "../include/records.h"
#include "account_index.h"
#include "audit.h"
#include "link_index.h"
#include "shm.h"
#include "wire.h"

namespace igp {

inline constexpr const char* kColdPrefix = "cold: ";

// Per-rank step counters shared by the ranks of one node (/dev/shm).
class StepClock {
 public:
  StepClock(const std::string& shm_name, int world, int rank, bool create);
  explicit StepClock(int world);  // process-private (tests: several cores in one process)
  int world() const { return world_; }
  int rank() const { return rank_; }
  void set_rank(int r) { rank_ = r; }
  void post(int64_t issued);                 // my issued-step count
  int64_t issued(int r) const;
  int64_t max_issued() const;
  void hold(int64_t gen);                    // I reached generation `gen` of a pause / stop
  bool all_hold(int64_t gen) const;
  int64_t hold_of(int r) const;
  void unlink_shared() { region_.unlink(); }

 private:
  struct alignas(64) Slot {
    std::atomic<int64_t> issued;
    std::atomic<int64_t> hold;
    char pad[48];
  };
  Region region_;
  Slot* slots_ = nullptr;
  int world_ = 1, rank_ = 0;
};

// stage times of one ScoreBatch call (ns): parse, resolve, queue (enqueue -> its first device
// step formed), device (first step formed -> every row back, incl. the copy out where rows are
// still staged; the in-place serialisation of the segments is NOT in it), serialize, total
struct CallTimings {
  int64_t parse = 0, resolve = 0, queue = 0, device = 0, serialize = 0, total = 0, rows = 0;
  int32_t seq_first = 0, seq_last = 0;  // the batch sequence numbers of the first / last step of its rows
};
// the calling thread's last score_batch / score_batch_view timings
inline CallTimings& last_timings_tl() {
  thread_local CallTimings t;
  return t;
}

struct ServeStats {
  int64_t items = 0, rows = 0, steps = 0, empty_steps = 0, unary = 0;
  int64_t parse_ns = 0, resolve_ns = 0, pack_ns = 0, device_ns = 0, copy_ns = 0, serialize_ns = 0, queue_ns = 0;
  int64_t submit_ns = 0, wait_errors = 0, max_step_rows = 0;
  // where a step's slot spends its cycle: device wait returned -> every segment finished (the
  // slot is free again), and the stepper's waits with rows queued: for the next slot (in-order
  // slots of the exchange) or for more rows (a step is formed at 7/8 full or after max_wait)
  int64_t release_ns = 0, slot_wait_ns = 0, rows_wait_ns = 0, slot_waits = 0, slot_wait_inflight = 0;
  // direct mode: steps whose rows the device read in place (a segment table, nothing copied) and
  // steps packed into the slot's request buffer (empty steps count as neither)
  int64_t inplace_steps = 0, packed_steps = 0;
  // request row buffers from the device (not reset): allocated now, and of those in the pool
  int64_t rowbufs = 0, rowbufs_free = 0;
  // cumulative decision counters (never reset)
  int64_t actions[4] = {0, 0, 0, 0};
  int64_t deciles[11] = {0};
  int64_t ml_high = 0, blacklisted = 0, scored = 0;
};

class ServeCore {
 public:
  struct Options {
    int max_wait_us = 200;       // a partial micro-batch waits at most this long for more rows
    int64_t timeout_us = -1;     // device wait deadline per step (-1: none)
    int finishers = 2;           // unary finisher threads
    bool features = true;        // responses carry the FeatureVector (risk.proto:73)
    int64_t stop_timeout_us = 30000000;
    int32_t seq0 = 0;            // batch sequence to continue from (dedup-ring rotation on device)
    // steps in flight while unary calls arrived in the last kUnaryWindowNs (0: the full depth):
    // deep pipelines serve bulk ScoreBatch traffic, but a unary call's step queues behind every
    // step ahead of it on the device (mixed traffic at depth 6 vs 4: abuse / tx p99 2.8-7.5 /
    // 2.4-16.6 vs 2.2-2.3 / 0.8-1.0 ms, profiles/r6/af). Direct (single-GPU) mode only: exchange
    // ranks issue their steps in lockstep
    int unary_depth = 0;
  };
  static constexpr int64_t kUnaryWindowNs = 20000000;

  // indexes: one per owner (world entries); dev: the device function table (owned by the
  // device object, which must outlive the core or be swapped out while paused); clock:
  // required when dev->exchange (shared with the peer ranks)
  ServeCore(std::vector<std::shared_ptr<AccountIndex>> indexes, const IgpDeviceOps* dev, int rank,
            std::shared_ptr<StepClock> clock, Options opt);
  ~ServeCore();
  ServeCore(const ServeCore&) = delete;
  ServeCore& operator=(const ServeCore&) = delete;

  // ScoreBatch: request bytes -> response bytes (blocking; callable from many threads)
  std::string score_batch(const char* data, size_t n, int64_t now, int64_t t0_ns);
  // the same, the response left in the calling thread's scratch buffer (valid until the
  // thread's next call): the native HTTP/2 server frames it from there
  std::string_view score_batch_view(const char* data, size_t n, int64_t now, int64_t t0_ns);
  // the same, serialised into a buffer of the caller's: alloc(upper_bound) -> buffer is called
  // exactly once, after parsing and resolving (not at all for a request without rows), with an
  // upper bound of the response size for the request's row count; returns the bytes written.
  // A null buffer fails the call. Nothing is enqueued before alloc returned, and a failed call
  // leaves no trace in the thread's next response
  using Alloc = std::function<char*(size_t)>;
  size_t score_batch_into(const char* data, size_t n, int64_t now, int64_t t0_ns, const Alloc& alloc);
  // pre-resolved rows (REQREC with slots; owners[] per row when world > 1): results in row order
  void score_rows(const ReqRec* rows, const int32_t* owners, size_t n, int64_t now, bool want_features,
                  ResultRec* res, FeatRec* feat);
  // unary ScoreTransaction: enqueue (non-blocking); the response comes back from poll() with `tag`
  void submit_tx(const char* data, size_t n, uint64_t tag, int64_t now, int64_t t0_ns);
  // many unary calls at once (the HTTP/2 worker hands over every call one read() delivered): one
  // batched account lookup, one queue lock and one stepper wake-up for all of them
  struct TxCall {
    const char* data;
    size_t n;
    uint64_t tag;
    int64_t t0_ns;
  };
  void submit_tx_many(const TxCall* calls, size_t n, int64_t now);
  // completed unary responses (tag, response bytes, error text: empty on success); blocks up
  // to timeout_us for the first one
  struct Done {
    uint64_t tag;
    std::string bytes;
    std::string err;
  };
  // error texts starting with kColdPrefix: no native core can serve the call (none attached on
  // the owner, or it is stopping): the ingress answers it through its cold (Python) path and
  // does NOT treat it as a core failure (h2grpc.cpp route_done, api/native_grpc.py _cold)
  size_t poll(std::vector<Done>& out, size_t max, int64_t timeout_us);
  // completions whose tag has bit 63 set go to `sink` (called on a finisher thread, must not
  // block) instead of the poll() queue: the native gRPC server (h2grpc.cpp) routes them back to
  // the connection that asked
  using Sink = std::function<void(std::vector<Done>&&)>;
  static constexpr uint64_t kSinkTag = uint64_t(1) << 63;
  void set_sink(Sink sink) {
    std::lock_guard<std::mutex> g(out_mu_);
    sink_ = std::move(sink);
  }

  // stop issuing new steps (exchange: every rank converges to the same step count) and wait
  // until every issued step completed; set_device() is allowed while paused
  void pause();
  void resume();
  void set_device(const IgpDeviceOps* dev);
  // drain and stop the threads (exchange: keeps following peers until every rank stopped)
  void stop();
  // failover: stop at once without converging with the peers; queued requests fail
  void abort();

  void set_links(std::shared_ptr<LinkIndex> links) { links_ = std::move(links); }
  // risk_scores audit: every result row the core hands back is appended to the ring, stamped
  // with the model version in force (set_model_version on every hot reload)
  void set_audit(std::shared_ptr<AuditRing> ring) { audit_ = std::move(ring); }
  void set_model_version(int v) { model_ver_.store(uint16_t(v)); }
  ServeStats stats(bool reset);
  int64_t issued() const { return issued_.load(); }
  int32_t seq() const { return seq_; }
  int late_steps() const { return late_.load(); }  // overran their deadline, not yet drained
  int world() const { return world_; }
  int pending_items();

  static int64_t now_ns();

 private:
  struct Item;
  struct Seg {
    Item* item;
    int32_t owner;       // exchange: chunk owner
    int32_t item_pos;    // first row in the item's (owner-sorted) row array
    int32_t dev_pos;     // direct: first row in the slot; exchange: first index in the owner's chunk
    int32_t count;
  };
  // One request's rows in host memory the device reads in place (device_ops.h host_alloc).
  // refs: the item that fills it + every step whose segment table names it; back to the pool
  // (or, once the pool moved on to another device or closed, freed) at zero
  struct RowBuf {
    ReqRec* rows = nullptr;
    uint64_t dev = 0;       // the address the device reads `rows` at
    size_t cap = 0;         // rows
    int64_t gen = 0;        // pool generation (set_device starts a new one)
    void (*free_fn)(void*) = nullptr;
    std::atomic<int> refs{0};
  };
  RowBuf* acquire_rowbuf(size_t n);   // null: the device has no in-place mode (or cannot allocate)
  void release_rowbuf(RowBuf* b);
  void drop_rowbuf(RowBuf* b);        // pool_mu_ held
  void close_pool(const IgpDeviceOps* next);
  struct Step {
    int slot = 0;
    int32_t seq = 0;
    int n = 0;
    bool wf = false;
    int64_t t_submit = 0, t_done = 0;
    std::vector<Seg> segs;
    std::vector<RowBuf*> bufs;  // in-place step: one reference per segment's buffer
    std::atomic<int> refs{0};
    bool failed = false;
    std::string err;
  };

  void stepper_loop();
  void note_wait(int64_t ServeStats::*field, int64_t ns);
  void completion_loop();
  void finisher_loop();
  void deliver(std::vector<Done>&& outs);
  void link_loop();
  void enqueue(Item* it);
  void wait_item(Item* it);
  bool issue_step(std::unique_lock<std::mutex>& lk, bool allow_empty);
  int next_slot_locked() const;
  void finish_seg(const Step& st, const Seg& s);
  void stream_seg(const Step& st, const Seg& s);
  void release_step_ref(Step* st);
  void resolve_rows(std::vector<wire::TxRow>& rows, Item* it);
  void converge(int64_t gen);
  void record_decisions(const ResultRec* r, int n);
  void audit_seg(const ResultRec* r, const ReqRec* rows, int owner, int n);

  std::vector<std::shared_ptr<AccountIndex>> idx_;
  const IgpDeviceOps* dev_;
  int world_, rank_;
  bool exchange_;
  int cap_, depth_;
  std::shared_ptr<StepClock> clock_;
  Options opt_;
  std::shared_ptr<LinkIndex> links_;
  std::shared_ptr<AuditRing> audit_;
  Sink sink_;
  std::atomic<uint16_t> model_ver_{1};

  // queue + slots (q_mu_)
  std::mutex q_mu_;
  std::condition_variable q_cv_;      // stepper: new items / free slot / peers / state
  std::deque<Item*> queue_;
  // unary calls (ScoreTransaction, one row each) form steps ahead of queued ScoreBatch rows:
  // under a saturating batch load a unary call otherwise waits behind every batch request
  // queued before it (mixed-traffic run, profiles/r6/d: ScoreTransaction p99 286 ms). Two
  // concurrent requests have no defined order between them (engine/dp.py ordering contract).
  std::deque<Item*> uqueue_;
  int64_t queued_rows_ = 0;
  std::vector<int> free_slots_;
  std::vector<std::unique_ptr<Step>> steps_;  // by slot
  int inflight_ = 0;
  int64_t last_unary_ns_ = 0;  // under q_mu_: the latest unary call's enqueue time
  bool stopping_ = false, stopped_ = false, paused_ = false, pause_req_ = false, aborting_ = false;
  int64_t hold_gen_ = 0;              // generation the stepper converges to (0: none)
  bool held_ = false;
  std::condition_variable idle_cv_;   // inflight_ reached 0 / paused

  // completion FIFO (c_mu_)
  std::mutex c_mu_;
  std::condition_variable c_cv_;
  std::deque<Step*> done_fifo_;
  bool c_stop_ = false;

  // unary finishing
  std::mutex f_mu_;
  std::condition_variable f_cv_;
  struct FTask {
    Step* step;
    std::vector<Seg> segs;
  };
  std::deque<FTask> ftasks_;
  bool f_stop_ = false;
  std::mutex out_mu_;
  std::condition_variable out_cv_;
  std::deque<Done> outq_;

  // links (background)
  std::mutex l_mu_;
  std::condition_variable l_cv_;
  // link inserts queued for the link thread: bounded, so the inserts a CheckBonusAbuse call
  // waits for (LinkIndex tickets) lag the ingress by at most a few ms; under overload batches
  // beyond it are not linked (links are best effort)
  static constexpr size_t kLinkQueue = 4;
  std::deque<std::pair<std::vector<uint64_t>, std::vector<int64_t>>> lq_;
  bool l_stop_ = false;

  // request row buffers (pool_mu_): free ones, most recently returned last
  std::mutex pool_mu_;
  std::vector<RowBuf*> pool_;
  int64_t pool_gen_ = 0, pool_live_ = 0;
  std::atomic<int64_t> pool_gen_now_{0};  // pool_gen_ for the stepper (no lock per step)
  bool pool_closed_ = false;

  std::atomic<int64_t> issued_{0};
  std::atomic<int> late_{0};
  int32_t seq_ = 0;
  int64_t gen_ = 0;  // pause / stop generations (clock hold)

  std::mutex st_mu_;
  ServeStats st_;
  std::atomic<int64_t> a_parse_{0}, a_resolve_{0}, a_serialize_{0}, a_copy_{0}, a_items_{0}, a_rows_{0};
  std::atomic<int64_t> dec_[11], act_[4], hi_{0}, bl_{0}, scored_{0};

  std::vector<std::thread> threads_;
};

}  // namespace igp
