// Per-row live windows of the masked (ONNX sequence_lens) K4 launches, shared by gru.hip and lstm.hip.
//
// A row with length L is updated on L steps and holds its state on every other one. With a zero
// initial state it does not matter where in the T-step window the L live steps sit, so each row
// gets a window [lo, hi) of actual time indices (after the reverse mapping t -> T-1-t):
//   dense input (mode 0):  [0, lens[row])            (lens == nullptr: [0, T))
//   event ring  (mode 1):  [T - min(ev_count, T), T)
// and an empty one for a slot of -1 or a row past the live count. One word per row:
// lo | (hi - lo) << 16, so the test is one subtract and one unsigned compare (T <= 65535, host-checked).
#pragma once
#include <stdint.h>

namespace igp {

// valid_from: the staging thread's first live time index (T for a row with nothing to read)
template <class Args>
__device__ __forceinline__ uint32_t seq_window(const Args& a, int grow, int n_live, int valid_from) {
  int hi = a.T;
  if (a.mode == 0 && a.lens && grow < n_live) hi = min(max(a.lens[grow], 0), a.T);
  return (uint32_t)valid_from | ((uint32_t)max(hi - valid_from, 0) << 16);
}

// One step's window test, handed to the layer steps. live(rt, r): is this lane's accumulator row
// rt * 16 + crow + r inside its window at the actual time index ta. The window word is read from
// LDS (wl[M]) where the select needs it, so nothing but two scalars lives through the MFMA loops:
// the 1024-thread instances have no vector register to spare. The unmasked kernels get the empty
// specialisation and compile to what they were.
template <int MASKED>
struct SeqLive {
  const uint32_t* wl;
  int crow, ta;
  __device__ __forceinline__ bool operator()(int rt, int r) const {
    const uint32_t w = wl[rt * 16 + crow + r];
    return (uint32_t)(ta - (int)(w & 0xffffu)) < (w >> 16);
  }
};
template <>
struct SeqLive<0> {};

}  // namespace igp
