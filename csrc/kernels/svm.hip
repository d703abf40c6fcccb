// Kernel machines on the f32 matrix cores (models/plan.py SVMStep): ai.onnx.ml SVMRegressor (SVR,
// one-class) and the two-class SVMClassifier,
//
//   dec[m] = sum_i coef[i] * K(x'_m, sv_i) + rho,   x' = x * in_scale + in_shift,   d = x' . sv_i
//   LINEAR d | POLY (gamma d + coef0)^degree | RBF exp(-gamma |x' - sv_i|^2) | SIGMOID tanh(gamma d + coef0)
//
// f32 throughout, whatever the plan's precision. One workgroup of four waves per tile of BM rows:
//  * the X tile is staged once into LDS with the input affine applied (one fma per element); for
//    RBF |x'|^2 is summed beside it, four lanes per row, in an order that depends on F alone;
//  * the support vectors stream through LDS in tiles of 64 vectors, 32 columns at a time, two
//    buffers: chunk t + 1 is loaded to registers under the MFMAs of chunk t;
//  * d comes from v_mfma_f32_16x16x4_f32 (the lane map of mfma4_f32, head_f32.h): exact f32 products summed in a
//    k order fixed by F. A wave owns 16 rows and NJ of the tile's four 16-column blocks, one
//    accumulator each (BM = 64: four blocks; BM = 32: two, the other two in the neighbour wave;
//    BM = 16: one, so a small bucket still gives every CU two workgroups);
//  * after the last chunk of a tile the C fragment goes through the kernel function (expf /
//    tanhf; POLY by square and multiply) and fmaf(coef, K, partial) adds it to the lane's partial
//    sum for (row, column block, column). RBF expands |x' - s|^2 = |x'|^2 + |s|^2 - 2 d; the host
//    centres x' and s for it (plan.py) and supplies |s|^2;
//  * at the end each (row, column block) partial is reduced over its 16 columns by an xor
//    butterfly, the four blocks meet in LDS and are added as (b0 + b1) + (b2 + b3). So a row's
//    sum runs in one order given S: its bucket, tile size and place in the tile do not matter.
//
// Padding: rows at or past the live count are staged as zeros and never stored; columns past F
// are zeros in both operands (written here and by the host, never read from X); a column of a
// tile past S is skipped by a select, not multiplied by a zero coefficient, since its kernel
// value may be inf (an RBF with negative gamma).
#include "common.h"
#include "head_f32.h"
#include "launch.h"

namespace igp {

namespace {

constexpr int SVM_SS = SVM_TILE_K + 4;  // chunk row stride in floats: rows 16 B apart in the bank row

__device__ __forceinline__ float svm_ipow(float t, int n) {
  float r = 1.f, b = t;
  while (n) {
    if (n & 1) r *= b;
    n >>= 1;
    if (n) b *= b;
  }
  return r;
}

template <int BM, int FP>
__global__ void __launch_bounds__(256) svm_kernel(SvmArgs a) {
  static_assert(BM == 16 || BM == 32 || BM == 64, "row tiles of 16, 32 or 64");
  constexpr int XS = FP + 4;   // X tile row stride in floats (as SVM_SS)
  constexpr int NJ = BM / 16;  // 16-column blocks per wave: the tile's four blocks go round its 64 / BM waves per row block
  __shared__ __attribute__((aligned(16))) float sX[BM * XS];
  __shared__ __attribute__((aligned(16))) float sS[2][SVM_TILE_S * SVM_SS];
  __shared__ float sXX[BM];
  __shared__ float sRed[BM][4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rb = wave * BM / 64;             // the wave's 16-row block
  const int j0 = (wave % (64 / BM)) * NJ;    // its first column block
  const int M = a.m_ptr ? min(*a.m_ptr, a.M) : a.M;
  const int row0 = blockIdx.x * BM;
  if (row0 >= M) return;
  const int F = a.F, S = a.S, fp = a.f_pad;
  const int nkc = fp / SVM_TILE_K, n_st = (S + SVM_TILE_S - 1) / SVM_TILE_S, total = n_st * nkc;

  for (int idx = tid; idx < BM * fp; idx += 256) {
    const int r = idx / fp, k = idx - r * fp;
    const int row = row0 + r;
    float v = 0.f;
    if (row < M && k < F) v = fmaf(a.X[(size_t)row * a.ldx + k], a.in_scale[k], a.in_shift[k]);
    sX[r * XS + k] = v;
  }
  __syncthreads();
  if (a.kernel == SVM_RBF && tid < BM * 4) {  // whole waves: BM * 4 is 64, 128 or 256
    const int r = tid >> 2, q = tid & 3;
    float s = 0.f;
    for (int k = 4 * q; k < fp; k += 16) {
      const float4 v = *reinterpret_cast<const float4*>(&sX[r * XS + k]);
      s = fmaf(v.x, v.x, s);
      s = fmaf(v.y, v.y, s);
      s = fmaf(v.z, v.z, s);
      s = fmaf(v.w, v.w, s);
    }
    s += __shfl_xor(s, 1, IGP_WAVE);
    s += __shfl_xor(s, 2, IGP_WAVE);
    if (q == 0) sXX[r] = s;
  }

  // chunk t of the table, this thread's two 16-byte pieces (c = 0, 1): rows (tid + 256 c) >> 3
  auto load_piece = [&](int t, int c) -> float4 {
    const int st = t / nkc, kc = t - st * nkc;
    const int ch = tid + c * 256;
    // the table is zero padded to [S_pad(64)][f_pad(32)]
    return *reinterpret_cast<const float4*>(a.sv + (size_t)(st * SVM_TILE_S + (ch >> 3)) * fp + kc * SVM_TILE_K + (ch & 7) * 4);
  };
  auto store_piece = [&](int buf, int c, float4 v) {
    const int ch = tid + c * 256;
    *reinterpret_cast<float4*>(&sS[buf][(ch >> 3) * SVM_SS + (ch & 7) * 4]) = v;
  };
  float4 rg0 = load_piece(0, 0), rg1 = load_piece(0, 1);  // named registers: an array here lands in scratch
  store_piece(0, 0, rg0);
  store_piece(0, 1, rg1);
  __syncthreads();

  float xx[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.kernel == SVM_RBF) {
#pragma unroll
    for (int q = 0; q < 4; ++q) xx[q] = sXX[rb * 16 + 4 * (lane >> 4) + q];
  }
  f32x4 acc[NJ];
  float part[NJ][4], cf[NJ], sn[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    cf[j] = sn[j] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) part[j][q] = 0.f;
  }
  const float* const xrow = &sX[(rb * 16 + (lane & 15)) * XS + 4 * (lane >> 4)];
  const float gamma = a.gamma, coef0 = a.coef0;

  int st = 0, kc = 0;
  for (int t = 0; t < total; ++t) {
    const int cur = t & 1;
    if (kc == 0) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int svi = st * SVM_TILE_S + (j0 + j) * 16 + (lane & 15);  // < S_pad
        cf[j] = a.coef[svi];
        if (a.kernel == SVM_RBF) sn[j] = a.sv_norm[svi];
      }
    }
    if (t + 1 < total) {  // global loads in flight under the MFMAs
      rg0 = load_piece(t + 1, 0);
      rg1 = load_piece(t + 1, 1);
    }
#pragma unroll
    for (int kk = 0; kk < SVM_TILE_K / 16; ++kk) {
      const float4 av = *reinterpret_cast<const float4*>(xrow + kc * SVM_TILE_K + kk * 16);
      float4 bv[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        bv[j] = *reinterpret_cast<const float4*>(
            &sS[cur][((j0 + j) * 16 + (lane & 15)) * SVM_SS + kk * 16 + 4 * (lane >> 4)]);
      // mfma4_f32's four steps, the accumulators interleaved: consecutive MFMAs are independent
      // (each accumulator still sees its k steps in the same order)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv[j].x, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv[j].y, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv[j].z, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv[j].w, acc[j], 0, 0, 0);
    }
    if (kc == nkc - 1) {  // the tile's dot products are complete: C[row 4 (lane >> 4) + q][column lane & 15]
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const bool live = st * SVM_TILE_S + (j0 + j) * 16 + (lane & 15) < S;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float d = acc[j][q];
          float kv;
          if (a.kernel == SVM_RBF) {
            float d2 = fmaf(-2.f, d, xx[q] + sn[j]);
            d2 = d2 < 0.f ? 0.f : d2;  // a NaN stays a NaN
            kv = expf(-gamma * d2);
          } else if (a.kernel == SVM_POLY) {
            kv = svm_ipow(fmaf(gamma, d, coef0), a.degree);
          } else if (a.kernel == SVM_SIGMOID) {
            kv = tanhf(fmaf(gamma, d, coef0));
          } else {
            kv = d;
          }
          if (live) part[j][q] = fmaf(cf[j], kv, part[j][q]);
        }
        acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if (t + 1 < total) {
      store_piece(cur ^ 1, 0, rg0);
      store_piece(cur ^ 1, 1, rg1);
    }
    __syncthreads();
    if (++kc == nkc) {
      kc = 0;
      ++st;
    }
  }

  // the 16 columns of each block: xor butterfly inside the 16-lane group (one order for every lane)
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = part[j][q];
      v += __shfl_xor(v, 1, IGP_WAVE);
      v += __shfl_xor(v, 2, IGP_WAVE);
      v += __shfl_xor(v, 4, IGP_WAVE);
      v += __shfl_xor(v, 8, IGP_WAVE);
      if ((lane & 15) == 0) sRed[rb * 16 + 4 * (lane >> 4) + q][j0 + j] = v;
    }
  __syncthreads();
  if (tid < BM) {
    const int row = row0 + tid;
    if (row < M) {
      const float dec = ((sRed[tid][0] + sRed[tid][1]) + (sRed[tid][2] + sRed[tid][3])) + a.rho;
      float v = dec;
      if (a.platt) {
        v = 1.f / (1.f + expf(a.prob_a * dec + a.prob_b));
        if (a.platt == 2) v = 1.f - v;
      }
      if (a.one_class) v = v > 0.f ? 1.f : -1.f;
      v = fmaf(v, a.post_scale, a.post_shift);
      a.Y[(size_t)row * a.ldy] = act_fn(v, a.act);
    }
  }
}

template <int BM>
void launch_bm(const SvmArgs& a, hipStream_t st) {
  const dim3 grid((a.M + BM - 1) / BM), block(256);
  if (a.f_pad <= 32) IGP_LAUNCH((svm_kernel<BM, 32>), grid, block, 0, st, a);
  else if (a.f_pad <= 64) IGP_LAUNCH((svm_kernel<BM, 64>), grid, block, 0, st, a);
  else if (a.f_pad <= 128) IGP_LAUNCH((svm_kernel<BM, 128>), grid, block, 0, st, a);
  else IGP_LAUNCH((svm_kernel<BM, SVM_MAX_F>), grid, block, 0, st, a);
}

}  // namespace

// the largest row tile that still gives each of the 256 CUs two workgroups (one wave per SIMD
// each: the second hides the first's barriers and LDS latency), down to 16 rows
int svm_tile(int M) { return M >= 64 * 512 ? 64 : M >= 32 * 512 ? 32 : 16; }

void launch_svm(const SvmArgs& a, hipStream_t st) {
  if (a.M <= 0) return;
  const int tile = a.tile ? a.tile : svm_tile(a.M);
  if (tile == 64) launch_bm<64>(a, st);
  else if (tile == 32) launch_bm<32>(a, st);
  else launch_bm<16>(a, st);
}

}  // namespace igp
