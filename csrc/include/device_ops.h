// C ABI between the native serving core (host runtime, _native: csrc/runtime/serve_core.cpp)
// and the device pipelines that execute its micro-batches:
//   * the single-GPU three-stream pipeline      (_hipk PipeDriver,  csrc/kernels/driver.hip)
//   * the owner-routed RCCL exchange pipeline   (_hipk XchgDriver,  csrc/kernels/exchange.hip)
//   * CPU shards                                 (_native CpuDevice / ShmXchgDevice, cpu_device.cpp)
// A plain function table keeps the two extension modules independent (no shared C++ types
// across the module boundary): a device hands out a pointer to its table, the core calls it
// from its own threads without the GIL.
#pragma once
#include <stdint.h>

#define IGP_DEVICE_OPS_ABI 5

// bits of IgpDeviceOps::submit's want_features argument
#define IGP_SUBMIT_WANT_FEATURES 1
#define IGP_SUBMIT_NO_UPDATE 2

// A step's rows read in place: at most IGP_ROW_SEGS runs of rows, each in host memory the device
// reads itself (host_alloc below), instead of one packed copy in the slot's request buffer.
// Sixteen covers one partial request from each of 16 ingress threads.
#define IGP_ROW_SEGS 16

#ifdef __cplusplus
extern "C" {
#endif

// One run of a step's rows: `count` ReqRec (48 bytes each) at the device-visible address `src`
// (16-byte aligned) are the step's rows first .. first + count - 1. The runs of a table are in
// row order and cover rows 0 .. n - 1 of the step without gaps.
typedef struct IgpRowSeg {
  uint64_t src;
  int32_t first;
  int32_t count;
} IgpRowSeg;

// The slot's segment table, next to its batch header in the request buffer. nseg == 0: the rows
// are in the slot's request buffer (rows()), as for every caller that knows nothing of the table.
typedef struct IgpRowSegTable {
  int32_t nseg;
  int32_t pad[3];
  IgpRowSeg seg[IGP_ROW_SEGS];
} IgpRowSegTable;

typedef struct IgpDeviceOps {
  uint32_t abi;       // IGP_DEVICE_OPS_ABI
  int32_t depth;      // pipeline slots (batches in flight)
  int32_t world;      // ranks of the exchange (1: single-shard pipeline)
  int32_t exchange;   // 0: rows = [cap] ReqRec of one batch; 1: rows = [world][cap + 1] ReqRec owner chunks
  int32_t cap;        // rows per batch (exchange: per-owner chunk capacity C)
  int32_t features_always;  // 1: results always carry FeatRec rows (exchange: fixed-size collectives)
  void* ctx;
  // the slot's host request buffer (pinned for GPU devices); valid once the slot's previous
  // batch was waited for
  char* (*rows)(void* ctx, int32_t slot);
  // launch the slot's batch: n live rows (exchange: ignored, counts ride in the chunk
  // headers), batch sequence number, scoring clock. Returns 0, or -1 with a message in err.
  // want_features is a set of IGP_SUBMIT_* bits: bit 0 asks for the FeatRec rows; bit 1 is the
  // caller's proof that no account has more than K1_SEG_MAX rows in this batch (mult_sketch.h),
  // so a device whose K1 applies those accounts itself may skip the multi-event update launch.
  // Devices without such a launch (CPU shards) and the exchange pipeline ignore bit 1.
  int32_t (*submit)(void* ctx, int32_t slot, int32_t n, int32_t seq, int64_t now, int32_t want_features, char* err,
                    int32_t errlen);
  // block until the slot's batch completed: 0 ok, 1 timeout (timeout_us >= 0), -1 error
  int32_t (*wait)(void* ctx, int32_t slot, int64_t timeout_us, char* err, int32_t errlen);
  // results of the slot's last batch. exchange == 0: ResultRec[n] and FeatRec[n] (features may
  // be null when not requested). exchange == 1: the returned chunks, [world][cap * W] bytes (or
  // res_owner_stride apart)
  // with W = 8 (+128 with features): cap ResultRec, then cap FeatRec per owner; features()
  // is unused.
  const void* (*results)(void* ctx, int32_t slot);
  const void* (*features)(void* ctx, int32_t slot);
  // exchange == 1: bytes from one owner's chunk to the next in results() (0: cap * W, the
  // chunks back to back). The per-GPU D2H result path hands out a node-shared region laid out
  // [owner][sender][cap * W], so a sender's chunks are world * cap * W apart.
  int64_t res_owner_stride;
  // In-place rows (optional, exchange == 0 only; any of the three null: the device has no such
  // mode and every step is packed into rows()).
  // host_alloc: `bytes` of host memory, 16-byte aligned, that the device reads in place (pinned
  // for GPU devices); *dev_addr receives the address the device reads it at. Null on failure.
  // host_free takes no ctx: it is a plain function of the device's module and stays callable for
  // a buffer after the device object that allocated it is gone (a device swapped out while
  // requests still hold their row buffers).
  void* (*host_alloc)(void* ctx, uint64_t bytes, uint64_t* dev_addr);
  void (*host_free)(void* p);
  // the slot's segment table (host-writable; same validity as rows()). The caller sets nseg for
  // EVERY step it submits once it has used the table: a slot keeps no state between steps.
  IgpRowSegTable* (*row_segs)(void* ctx, int32_t slot);
} IgpDeviceOps;

#ifdef __cplusplus
}
#endif
