// Row ops on one [M][N] activation tensor (models/plan.py RowStep): what the MFMA kernels'
// epilogues do not carry.
//
//   op 0 (layernorm)  Y[r] = (X[r] - mean) / sqrt(var + eps) * gamma + beta      (beta nullable)
//                     two passes over the row held in registers: the mean, then the sum of squared
//                     deviations from it (not E[x^2] - mean^2)
//   op 1 (softmax)    Y[r] = exp(X[r] - max) / sum(exp(X[r] - max))
//   op 2 (act)        Y = act(X) elementwise: relu, sigmoid, tanh, leaky_relu, elu, selu, softplus,
//                     hard_sigmoid, gelu (erf; erfc in the negative tail), gelu_tanh, clip, prelu (one
//                     slope, or one per column through gamma); overflow-safe forms throughout
//
// All three are memory-bound. The two reductions run one wave per row, four rows per 256-thread
// block, with no LDS and no barrier (a wave whose row is past the live count just exits). Lane l
// holds the 4 consecutive elements (j * 64 + l) * 4 .. + 3 of the row for j < V, V = 1 / 2 / 4
// for N <= 256 / 512 / 1024, so the row is read from memory once; wider rows take the looped kernel,
// which re-reads the row (from L2) per pass. A 4-element chunk is one load when the row stride and
// base keep it aligned (f32: 16 bytes, ld % 4 == 0; bf16: 8 bytes, ld % 4 == 0) and lies inside N;
// otherwise, and for the chunk holding the end of the row, its elements are loaded one by one.
// Elements past N are never loaded or stored: they enter the reductions as the identity (0, or
// -inf for the maximum), so a stride wider than N may hold anything. X and Y are f32 or bf16 (the
// producer's / consumer's activation dtype); all math is f32. Live rows come from m_ptr when the
// step is replayed from a graph.
#include "common.h"
#include "launch.h"

namespace igp {

namespace {

// elements [c0, c0 + 4) of a row; those at or past N are `fill`
__device__ __forceinline__ void load4(const void* row, int bf16, bool vec, int c0, int N, float fill, float (&v)[4]) {
  if (vec && c0 + 4 <= N) {
    if (bf16) {
      const uint2 u = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(row) + c0);
      v[0] = __uint_as_float(u.x << 16);
      v[1] = __uint_as_float(u.x & 0xffff0000u);
      v[2] = __uint_as_float(u.y << 16);
      v[3] = __uint_as_float(u.y & 0xffff0000u);
    } else {
      const float4 f = *reinterpret_cast<const float4*>(static_cast<const float*>(row) + c0);
      v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = fill;
    if (c0 + k < N)
      v[k] = bf16 ? bf16_to_f32(static_cast<const uint16_t*>(row)[c0 + k]) : static_cast<const float*>(row)[c0 + k];
  }
}

__device__ __forceinline__ void store4(void* row, int bf16, bool vec, int c0, int N, const float (&v)[4]) {
  if (vec && c0 + 4 <= N) {
    if (bf16) {
      uint2 u;
      u.x = uint32_t(f32_to_bf16(v[0])) | (uint32_t(f32_to_bf16(v[1])) << 16);
      u.y = uint32_t(f32_to_bf16(v[2])) | (uint32_t(f32_to_bf16(v[3])) << 16);
      *reinterpret_cast<uint2*>(static_cast<uint16_t*>(row) + c0) = u;
    } else {
      *reinterpret_cast<float4*>(static_cast<float*>(row) + c0) = make_float4(v[0], v[1], v[2], v[3]);
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c0 + k < N) {
      if (bf16) static_cast<uint16_t*>(row)[c0 + k] = f32_to_bf16(v[k]);
      else static_cast<float*>(row)[c0 + k] = v[k];
    }
}

// whether 4-element chunks of rows `ld` apart starting at p are aligned for one load / store
__device__ __forceinline__ bool chunk_aligned(const void* p, int ld, int bf16) {
  return (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & (bf16 ? 7u : 15u)) == 0;
}

__device__ __forceinline__ const void* row_ptr(const void* p, int bf16, int r, int ld) {
  return static_cast<const char*>(p) + size_t(r) * size_t(ld) * (bf16 ? 2 : 4);
}

__device__ __forceinline__ float row_act(int act, float x, float p0, float p1, float slope) {
  switch (act) {
    case RA_RELU: return x > 0.f ? x : 0.f;
    case RA_SIGMOID: return sigmoid_precise(x);
    case RA_TANH: return tanhf(x);
    case RA_LEAKY_RELU: return x > 0.f ? x : p0 * x;
    case RA_ELU: return x > 0.f ? x : p0 * expm1f(x);
    case RA_SELU: return p1 * (x > 0.f ? x : p0 * expm1f(x));
    case RA_SOFTPLUS: return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
    case RA_HARD_SIGMOID: return fminf(1.f, fmaxf(0.f, fmaf(p0, x, p1)));
    // x * Phi(x): 1 + erf cancels for x < 0, where erfc gives the same tail to full precision
    case RA_GELU:
      return x >= 0.f ? 0.5f * x * (1.f + erff(x * 0.70710678118654752f)) : 0.5f * x * erfcf(-x * 0.70710678118654752f);
    // 0.5 x (1 + tanh(u)) = x * sigmoid(2u), without the cancellation of 1 + tanh in the negative
    // tail; past exp(20) the 1 is below f32 resolution and x * exp(-a) cannot overflow
    case RA_GELU_TANH: {
      const float a = -1.59576912160573071f * (x + 0.044715f * x * x * x);
      return a > 20.f ? x * expf(-a) : x / (1.f + expf(a));
    }
    case RA_CLIP: return fminf(fmaxf(x, p0), p1);
    case RA_PRELU: return x >= 0.f ? x : slope * x;
    default: return x;
  }
}

// One wave per row, the row in V float4 per lane (N <= 256 * V).
template <int V>
__global__ void __launch_bounds__(256) row_reduce_kernel(RowArgs a) {
  const int M = a.m_ptr ? min(*a.m_ptr, a.M) : a.M;
  const int N = a.N;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  if (r >= M) return;
  const void* x = row_ptr(a.X, a.x_bf16, r, a.ldx);
  void* y = const_cast<void*>(row_ptr(a.Y, a.y_bf16, r, a.ldy));
  const bool xv = chunk_aligned(a.X, a.ldx, a.x_bf16), yv = chunk_aligned(a.Y, a.ldy, a.y_bf16);
  const bool softmax = a.op == ROW_SOFTMAX;
  float v[V][4];
#pragma unroll
  for (int j = 0; j < V; ++j) load4(x, a.x_bf16, xv, (j * 64 + lane) * 4, N, softmax ? -INFINITY : 0.f, v[j]);
  if (softmax) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) m = fmaxf(m, v[j][k]);
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[j][k] = (j * 64 + lane) * 4 + k < N ? expf(v[j][k] - m) : 0.f;
        s += v[j][k];
      }
    s = wave_sum(s);
#pragma unroll
    for (int j = 0; j < V; ++j) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[j][k] = v[j][k] / s;
      store4(y, a.y_bf16, yv, (j * 64 + lane) * 4, N, v[j]);
    }
    return;
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < V; ++j) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
  const float mean = wave_sum(s) / float(N);
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < V; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[j][k] = (j * 64 + lane) * 4 + k < N ? v[j][k] - mean : 0.f;
      ss += v[j][k] * v[j][k];
    }
  const float inv = 1.f / sqrtf(wave_sum(ss) / float(N) + a.eps);
  const bool gv = chunk_aligned(a.gamma, 4, 0), bv = chunk_aligned(a.beta, 4, 0);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int c0 = (j * 64 + lane) * 4;
    if (c0 >= N) continue;
    float g[4], b[4] = {0.f, 0.f, 0.f, 0.f};
    load4(a.gamma, 0, gv, c0, N, 0.f, g);
    if (a.beta) load4(a.beta, 0, bv, c0, N, 0.f, b);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[j][k] = v[j][k] * inv * g[k] + b[k];
    store4(y, a.y_bf16, yv, c0, N, v[j]);
  }
}

// One wave per row of any width: the row is re-read for every pass (mean / squared deviations /
// write; maximum / sum / write).
__global__ void __launch_bounds__(256) row_reduce_loop_kernel(RowArgs a) {
  const int M = a.m_ptr ? min(*a.m_ptr, a.M) : a.M;
  const int N = a.N;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  if (r >= M) return;
  const void* x = row_ptr(a.X, a.x_bf16, r, a.ldx);
  void* y = const_cast<void*>(row_ptr(a.Y, a.y_bf16, r, a.ldy));
  const bool xv = chunk_aligned(a.X, a.ldx, a.x_bf16), yv = chunk_aligned(a.Y, a.ldy, a.y_bf16);
  float v[4];
  if (a.op == ROW_SOFTMAX) {
    float m = -INFINITY, s = 0.f;
    for (int c0 = lane * 4; c0 < N; c0 += 256) {
      load4(x, a.x_bf16, xv, c0, N, -INFINITY, v);
      m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
    m = wave_max(m);
    for (int c0 = lane * 4; c0 < N; c0 += 256) {
      load4(x, a.x_bf16, xv, c0, N, -INFINITY, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) s += c0 + k < N ? expf(v[k] - m) : 0.f;
    }
    s = wave_sum(s);
    for (int c0 = lane * 4; c0 < N; c0 += 256) {
      load4(x, a.x_bf16, xv, c0, N, -INFINITY, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = expf(v[k] - m) / s;
      store4(y, a.y_bf16, yv, c0, N, v);
    }
    return;
  }
  float s = 0.f, ss = 0.f;
  for (int c0 = lane * 4; c0 < N; c0 += 256) {
    load4(x, a.x_bf16, xv, c0, N, 0.f, v);
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float mean = wave_sum(s) / float(N);
  for (int c0 = lane * 4; c0 < N; c0 += 256) {
    load4(x, a.x_bf16, xv, c0, N, 0.f, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = c0 + k < N ? v[k] - mean : 0.f;
      ss += d * d;
    }
  }
  const float inv = 1.f / sqrtf(wave_sum(ss) / float(N) + a.eps);
  const bool gv = chunk_aligned(a.gamma, 4, 0), bv = chunk_aligned(a.beta, 4, 0);
  for (int c0 = lane * 4; c0 < N; c0 += 256) {
    float g[4], b[4] = {0.f, 0.f, 0.f, 0.f};
    load4(x, a.x_bf16, xv, c0, N, 0.f, v);
    load4(a.gamma, 0, gv, c0, N, 0.f, g);
    if (a.beta) load4(a.beta, 0, bv, c0, N, 0.f, b);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (v[k] - mean) * inv * g[k] + b[k];
    store4(y, a.y_bf16, yv, c0, N, v);
  }
}

// Elementwise: one thread per 4 consecutive elements of a row, consecutive threads on consecutive
// chunks, so a wave reads / writes whole 1 KiB (f32) runs of a row.
__global__ void __launch_bounds__(256) row_act_kernel(RowArgs a) {
  const int M = a.m_ptr ? min(*a.m_ptr, a.M) : a.M;
  const int N = a.N;
  const int chunks = (N + 3) >> 2;
  const long e = long(blockIdx.x) * 256 + threadIdx.x;
  const int r = int(e / chunks), c0 = int(e - long(r) * chunks) * 4;
  if (r >= M) return;
  const bool xv = chunk_aligned(a.X, a.ldx, a.x_bf16), yv = chunk_aligned(a.Y, a.ldy, a.y_bf16);
  float v[4], sl[4] = {a.p0, a.p0, a.p0, a.p0};
  load4(row_ptr(a.X, a.x_bf16, r, a.ldx), a.x_bf16, xv, c0, N, 0.f, v);
  if (a.act == RA_PRELU && a.gamma) load4(a.gamma, 0, chunk_aligned(a.gamma, 4, 0), c0, N, 0.f, sl);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = row_act(a.act, v[k], a.p0, a.p1, sl[k]);
  store4(const_cast<void*>(row_ptr(a.Y, a.y_bf16, r, a.ldy)), a.y_bf16, yv, c0, N, v);
}

}  // namespace

void launch_row(const RowArgs& a, hipStream_t st) {
  if (a.M <= 0 || a.N <= 0) return;
  if (a.op == ROW_ACT) {
    const long n = long(a.M) * ((a.N + 3) / 4);
    IGP_LAUNCH(row_act_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, a);
    return;
  }
  const dim3 grid(unsigned((a.M + 3) / 4)), block(256);
  if (a.N <= 256) IGP_LAUNCH(row_reduce_kernel<1>, grid, block, 0, st, a);
  else if (a.N <= 512) IGP_LAUNCH(row_reduce_kernel<2>, grid, block, 0, st, a);
  else if (a.N <= 1024) IGP_LAUNCH(row_reduce_kernel<4>, grid, block, 0, st, a);
  else IGP_LAUNCH(row_reduce_loop_kernel, grid, block, 0, st, a);
}

}  // namespace igp
