// Layer-1 input staging of the K4 kernels (gru.hip, lstm.hip, gru_ws.hip, gru_wsx.hip): where a
// row's sequence comes from and how one 8-element chunk of x_t is read, as bf16 or as a bf16
// (hi, lo) pair. Templated on the args struct like seq_window.h, so GruArgs and LstmArgs both fit.
#pragma once
#include <stdint.h>

#include "common.h"

namespace igp {

// hi = bf16(x), lo = bf16(x - hi): the pair of the f32-faithful split mode
__device__ __forceinline__ void bf16_split(float x, uint16_t& hi, uint16_t& lo) {
  hi = f32_to_bf16(x);
  lo = f32_to_bf16(x - __uint_as_float((uint32_t)hi << 16));
}

__device__ __forceinline__ uint4 bf16_pack8(const uint16_t (&v)[8]) {
  return make_uint4(v[0] | (uint32_t)v[1] << 16, v[2] | (uint32_t)v[3] << 16, v[4] | (uint32_t)v[5] << 16,
                    v[6] | (uint32_t)v[7] << 16);
}

// A row's source: its event-ring slot and head (mode 1) and the first live logical time index
// (`from`; T for a row with nothing to read: a slot of -1 or a row past the live count).
struct SeqSrc {
  int slot, head, from;
};

template <class Args>
__device__ __forceinline__ SeqSrc seq_src(const Args& a, int grow, int n_live) {
  SeqSrc s = {-1, 0, a.T};
  if (grow < n_live) {
    if (a.mode == 1) {
      s.slot = a.slots[grow];
      if (s.slot >= 0) {
        const AcctRT r = a.rt[s.slot];
        s.head = r.ev_head;
        s.from = a.T - min(r.ev_count, a.T);
      }
    } else {
      s.from = 0;
    }
  }
  return s;
}

// The source as two LDS words {slot, head | from << 16}: the cluster kernels keep it there so
// that their layer-2 waves carry no staging registers (T < 32768 and ev_ring <= 65535, checked by
// gru_ws_eligible / gru_wsx_eligible).
__device__ __forceinline__ int2 seq_src_pack(const SeqSrc& s) { return make_int2(s.slot, s.head | (s.from << 16)); }
__device__ __forceinline__ SeqSrc seq_src_unpack(int2 m) { return {m.x, m.y & 0xffff, m.y >> 16}; }

// Logical step t -> the time index to read (direction=reverse runs forward over the time-reversed
// sequence); false when there is nothing to read: past the end, or before the row's first live step.
template <class Args>
__device__ __forceinline__ bool seq_time(const Args& a, const SeqSrc& s, int& t) {
  if (t >= a.T) return false;
  if (a.reverse) t = a.T - 1 - t;
  return t >= s.from;
}

// chunk q of time index t in the row's event ring (bf16 values)
template <class Args>
__device__ __forceinline__ uint4 seq_ring_chunk(const Args& a, const SeqSrc& s, int q, int t) {
  int idx = (s.head - a.T + t) % a.ev_ring;
  if (idx < 0) idx += a.ev_ring;
  return *reinterpret_cast<const uint4*>(a.ev + (((size_t)s.slot * a.ev_ring + idx) * a.I + q * 8));
}

template <class Args>
__device__ __forceinline__ void seq_dense_chunk(const Args& a, int grow, int q, int t, float (&f)[8]) {
  const float* src = a.X + (((size_t)t * a.x_rows + grow) * a.I + q * 8);
  const float4 f0 = *reinterpret_cast<const float4*>(src);
  const float4 f1 = *reinterpret_cast<const float4*>(src + 4);
  f[0] = f0.x, f[1] = f0.y, f[2] = f0.z, f[3] = f0.w;
  f[4] = f1.x, f[5] = f1.y, f[6] = f1.z, f[7] = f1.w;
}

// Chunk q (8 elements) of row `grow` at logical step t as bf16 x 8; zero where there is nothing to read.
template <class Args>
__device__ __forceinline__ uint4 seq_load(const Args& a, const SeqSrc& s, int grow, int q, int t) {
  if (!seq_time(a, s, t)) return make_uint4(0, 0, 0, 0);
  if (a.mode == 1) return seq_ring_chunk(a, s, q, t);
  float f[8];
  uint16_t h[8];
  seq_dense_chunk(a, grow, q, t, f);
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] = f32_to_bf16(f[e]);
  return bf16_pack8(h);
}

// The same chunk as a (hi, lo) pair: the event ring holds bf16 values (lo = 0), dense f32 input splits.
template <class Args>
__device__ __forceinline__ void seq_load_split(const Args& a, const SeqSrc& s, int grow, int q, int t, uint4& hi,
                                               uint4& lo) {
  hi = lo = make_uint4(0, 0, 0, 0);
  if (!seq_time(a, s, t)) return;
  if (a.mode == 1) {
    hi = seq_ring_chunk(a, s, q, t);
    return;
  }
  float f[8];
  uint16_t h[8], l[8];
  seq_dense_chunk(a, grow, q, t, f);
#pragma unroll
  for (int e = 0; e < 8; ++e) bf16_split(f[e], h[e], l[e]);
  hi = bf16_pack8(h);
  lo = bf16_pack8(l);
}

}  // namespace igp
