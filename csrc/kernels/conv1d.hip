// Temporal convolutions on the f32 matrix cores (models/plan.py ConvStep / SeqPoolStep): one layer of
// a Conv1D / TCN sequence model per launch,
//
//   out[row][t][o] = act_post( act( b[o] + sum_j sum_c W[o][c][j] * x[row][t - pad_left + j dil][c] ) + res[row][t][o] )
//
// with x zero outside [0, T). f32 throughout, whatever the plan's precision. Activations live in
// global memory channel-last, [rows][T][ld] f32 with ld a multiple of 4.
//
// One workgroup of four waves per (row, tile of `tt` = 64 or 32 time steps):
//  * the tile's input steps [t0 - pad_left, t0 - pad_left + tt + dil (k - 1)) are staged once into LDS,
//    channels padded to a multiple of 16 with zeros; steps outside [0, T) - and, for the event rings,
//    before the row's live window - are staged as zeros. That halo is the only place padding exists;
//    no im2col is formed. Where tile plus halo does not fit the 64 KiB (wide layers with a long
//    dilation), tap j's tt steps are staged before tap j instead (`per_tap`); the arithmetic is the same;
//  * the layer is the implicit GEMM out^T [C_out][tt] = W [C_out][k C_in] x im2col [k C_in][tt] on
//    v_mfma_f32_16x16x4_f32 (the lane map of mfma4_f32, head_f32.h), weights as the A operand: a lane
//    then holds four consecutive output channels of one time step, so the epilogue loads the bias and
//    the residual and stores the result as 16-byte vectors. A wave owns units of 16 output channels x
//    32 time steps (two independent accumulators), taken round-robin; the B fragment of reduction
//    index (j, c) and step t is LDS row t - pad_left + j dil of the staged tile;
//  * the weights are fragment-packed on the host (plan.conv_tables): one wave load is 1 KiB
//    contiguous, streamed from L2;
//  * an output element is summed in one fixed order: taps j ascending, inside a tap the channels in
//    chunks of 16 ascending, k-steps of four inside a chunk. It depends on (k, C_in) alone, so a row's
//    result does not depend on the bucket, on its workgroup or place in a tile, on tt or on per_tap.
//
// First layers read (mode 0) the dense model input [T][x_rows][I] f32 or (mode 1) the store's event
// rings through `slots`, by the seq_src / seq_ring_chunk rules of seq_input.h: the window
// [T - min(ev_count, T), T) of the ring ending at ev_head, bf16 widened exactly, zeros before it and
// for slot -1. Later layers (mode 2) read an activation buffer. Rows at or past the live count are
// neither read nor stored. The output columns past C_out of its last 16-channel block are written as
// zeros, any further padding column is left alone: no reader looks past its channel count.
//
// seq_pool: [rows][T][ld] -> [rows][>= C], f32 or bf16: last copies step T - 1; mean, sum and max run
// over t ascending (one order per element); a NaN in the column makes max NaN, as in the executor
// (csrc/runtime/conv.cpp).
#include "common.h"
#include "head_f32.h"
#include "launch.h"
#include "seq_input.h"

namespace igp {

namespace {

constexpr int CONV_LDS = 16384;   // most floats a workgroup stages: 64 KiB (the launch asks for what the tile needs)

__global__ void __launch_bounds__(256) conv1d_kernel(ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sX[];   // n_stage * xs floats (launch_conv1d)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int n_live = a.m_ptr ? min(*a.m_ptr, a.n_rows) : a.n_rows;
  const int n_tt = (a.T + a.tt - 1) / a.tt;
  const int row = blockIdx.x / n_tt, t0 = (blockIdx.x - row * n_tt) * a.tt;
  if (row >= n_live) return;
  // LDS row stride xs: the channels padded to 16, plus 4 so that rows lie 16 B apart in the bank row
  const int cp = (a.c_in + 15) & ~15, xs = cp + 4, c4n = cp >> 2, n_kc = cp >> 4;
  const int span = a.dil * (a.k - 1);
  const int n_stage = a.per_tap ? a.tt : a.tt + span;
  if (n_stage * xs > CONV_LDS) return;   // the launch checks this; never index past the tile
  const SeqSrc src = seq_src(a, row, n_live);   // modes 0 and 2: every step is live

  // input steps [t_base, t_base + nr) of the row, all channels, into LDS rows [0, nr)
  auto stage = [&](int t_base, int nr) {
    for (int idx = tid; idx < nr * c4n; idx += 256) {
      const int r = idx / c4n, c = (idx - r * c4n) * 4;
      const int t = t_base + r;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (t >= src.from && t < a.T && c < a.c_in) {
        if (a.mode == 2) {
          const float4 f = *reinterpret_cast<const float4*>(a.X + ((size_t)row * a.T + t) * a.ldx + c);
          v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        } else if (a.mode == 1) {
          int ri = (src.head - a.T + t) % a.ev_ring;   // seq_ring_chunk's index
          if (ri < 0) ri += a.ev_ring;
          const uint2 h = *reinterpret_cast<const uint2*>(a.ev + (((size_t)src.slot * a.ev_ring + ri) * a.I + c));
          v[0] = bf16_to_f32((uint16_t)(h.x & 0xffff)), v[1] = bf16_to_f32((uint16_t)(h.x >> 16));
          v[2] = bf16_to_f32((uint16_t)(h.y & 0xffff)), v[3] = bf16_to_f32((uint16_t)(h.y >> 16));
        } else {
          const float* p = a.X + ((size_t)t * a.x_rows + row) * a.c_in + c;
          if ((a.c_in & 3) == 0) {   // rows of the dense input are then 16-byte aligned
            const float4 f = *reinterpret_cast<const float4*>(p);
            v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c + e < a.c_in) v[e] = p[e];
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c + e >= a.c_in) v[e] = 0.f;
      }
      *reinterpret_cast<float4*>(&sX[r * xs + c]) = make_float4(v[0], v[1], v[2], v[3]);
    }
  };

  if (!a.per_tap) {
    stage(t0 - a.pad_left, n_stage);
    __syncthreads();
  }
  const int n_ob = (a.c_out + 15) >> 4, n_tg = a.tt >> 5, units = n_ob * n_tg;
  for (int u0 = 0; u0 < units; u0 += 4) {   // a round: one unit per wave (the barriers below are workgroup-uniform)
    const int u = u0 + wave;
    const int ob = u / n_tg, tg = u - ob * n_tg;
    const bool work = u < units && t0 + tg * 32 < a.T;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < a.k; ++j) {
      if (a.per_tap) {
        // (staged once per round and tap: a wide layer - up to 16 channel blocks at tt = 32, four
        // rounds - stages each tap four times. Keeping every round's accumulators live across the tap
        // loop would stage once; not done, this path is the rare wide-and-long-dilation shape)
        __syncthreads();   // the previous tap's readers are done
        stage(t0 - a.pad_left + j * a.dil, n_stage);
        __syncthreads();
      }
      if (!work) continue;
      const float* xb = &sX[(tg * 32 + li + (a.per_tap ? 0 : j * a.dil)) * xs + 4 * g];
      const float4* wp = reinterpret_cast<const float4*>(a.W) + (size_t)(ob * a.k + j) * n_kc * 64 + lane;
#pragma unroll 2
      for (int kc = 0; kc < n_kc; ++kc) {
        const float4 av = wp[kc * 64];
        const float4 b0 = *reinterpret_cast<const float4*>(xb + kc * 16);
        const float4 b1 = *reinterpret_cast<const float4*>(xb + 16 * xs + kc * 16);
        // mfma4_f32's four steps on two independent accumulators
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b0.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, b0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, b1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, b0.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, b1.w, acc1, 0, 0, 0);
      }
    }
    if (!work) continue;
    // C fragment: output channels ob 16 + 4 g + q of step (lane & 15) of each 16-step block
    const int o0 = ob * 16 + 4 * g;
    if (o0 >= a.ldy) continue;
    const float4 bv = *reinterpret_cast<const float4*>(a.bias + o0);
    const float bq[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int t = t0 + tg * 32 + nt * 16 + li;
      if (t >= a.T) continue;
      const f32x4 acc = nt ? acc1 : acc0;
      float rq[4] = {0.f, 0.f, 0.f, 0.f};
      if (a.res && o0 < a.c_out) {
        const float4 r = *reinterpret_cast<const float4*>(a.res + ((size_t)row * a.T + t) * a.ldr + o0);
        rq[0] = r.x, rq[1] = r.y, rq[2] = r.z, rq[3] = r.w;
      }
      float y[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v = act_fn(acc[q] + bq[q], a.act);
        if (a.res) v += rq[q];
        v = act_fn(v, a.act_post);
        y[q] = o0 + q < a.c_out ? v : 0.f;
      }
      *reinterpret_cast<float4*>(a.Y + ((size_t)row * a.T + t) * a.ldy + o0) = make_float4(y[0], y[1], y[2], y[3]);
    }
  }
}

__global__ void __launch_bounds__(256) seq_pool_kernel(SeqPoolArgs a) {
  const int n_live = a.m_ptr ? min(*a.m_ptr, a.n_rows) : a.n_rows;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int row = (int)(idx / a.C), c = (int)(idx - (long long)row * a.C);
  if (row >= n_live) return;
  const float* x = a.X + (size_t)row * a.T * a.ldx + c;
  float v;
  if (a.op == POOL_LAST) {
    v = x[(size_t)(a.T - 1) * a.ldx];
  } else if (a.op == POOL_MAX) {
    v = x[0];
    for (int t = 1; t < a.T; ++t) {
      const float e = x[(size_t)t * a.ldx];
      v = v != v ? v : (e != e || e > v) ? e : v;   // a NaN in the column gives NaN
    }
  } else {
    v = 0.f;
    for (int t = 0; t < a.T; ++t) v += x[(size_t)t * a.ldx];
    if (a.op == POOL_MEAN) v /= (float)a.T;
  }
  if (a.y_bf16) reinterpret_cast<uint16_t*>(a.Y)[(size_t)row * a.ldy + c] = f32_to_bf16(v);
  else reinterpret_cast<float*>(a.Y)[(size_t)row * a.ldy + c] = v;
}

}  // namespace

bool conv1d_plan(const ConvArgs& a, int& tt, int& per_tap) {
  const int xs = ((a.c_in + 15) & ~15) + 4, span = a.dil * (a.k - 1);
  tt = a.tt ? a.tt : (64 * xs <= CONV_LDS ? 64 : 32);
  if (tt * xs > CONV_LDS) return false;
  per_tap = a.per_tap || (tt + span) * xs > CONV_LDS;
  return true;
}

void launch_conv1d(const ConvArgs& a0, hipStream_t st) {
  if (a0.n_rows <= 0 || a0.T <= 0) return;
  ConvArgs a = a0;
  if (!conv1d_plan(a0, a.tt, a.per_tap)) return;   // the binding refuses such a launch
  const int n_tt = (a.T + a.tt - 1) / a.tt;
  // LDS for the staged steps only: a 64-channel layer takes 22 KiB, so several workgroups share a CU
  const int xs = ((a.c_in + 15) & ~15) + 4, n_stage = a.per_tap ? a.tt : a.tt + a.dil * (a.k - 1);
  IGP_LAUNCH(conv1d_kernel, dim3((unsigned)(a.n_rows * n_tt)), dim3(256), (size_t)n_stage * xs * sizeof(float), st, a);
}

void launch_seq_pool(const SeqPoolArgs& a, hipStream_t st) {
  if (a.n_rows <= 0 || a.C <= 0) return;
  const long long total = (long long)a.n_rows * a.C;
  IGP_LAUNCH(seq_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace igp
