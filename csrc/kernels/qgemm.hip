// K3 quantised dense layers on the CDNA4 i8 matrix cores (QDQ models, models/plan.py QDenseStep):
//
//   acc[m][n] = sum_k X[m][k] * W[n][k]                      (int8 x int8 -> int32, exact)
//   v         = float(acc + corr[n]) * mult[n] + bias[n]     (then the activation)
//   Y         = v as f32 / bf16, or the requantised byte clamp(rintf(v / s_y) + z_y) - off_y
//
// A quantised value q of type uint8 / int8 is stored as the signed byte q - off (off = 128 / 0;
// for uint8 that is the byte XOR 0x80), so both operand types feed v_mfma_i32_16x16x64_i8 as they
// are; corr[n] = (off_x - z_x) * sum_k W[n][k] puts the activation zero point back. W holds
// w_q - z_w, zero padded to [N_pad(128)][K_pad(64)]: bytes of X past K multiply zeros.
//
// Same blocking as gemm_kernel (gemm.hip): 256 threads, 4 waves 2 x 2, two LDS buffers of
// BK = 128 bytes per row (+16 of padding: the bf16 kernel's 144-byte rows), tile k+1 loaded to
// registers under the MFMAs of tile k. Each lane hands the MFMA 16 consecutive k bytes of row
// (lane & 15) at k offset 16 (lane >> 4), for A and B alike: the integer sum is order-free, so any
// k order the instruction gives the 64 bytes is the same for both operands and drops out; the
// C/D map is the dtype-independent one (col = lane & 15, row = 4 (lane >> 4) + reg).
#include "common.h"
#include "head_f32.h"
#include "launch.h"

namespace igp {

typedef __attribute__((ext_vector_type(4))) int i32x4;

constexpr int QG_BK = 128;   // k bytes per tile: two MFMA k-steps
constexpr int QG_PAD = 16;

__device__ __forceinline__ bool aligned16(const void* p, int ld_bytes) {
  return ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)(unsigned)ld_bytes) & 15) == 0;
}

// the stored signed byte of quantize(v): clamp(rintf(v / s) + z, type range) - off. A true IEEE
// division (no reciprocal) and round half to even, as QuantizeLinear specifies.
__device__ __forceinline__ int quant_byte(float v, float s, int zp, int off) {
  const float q = rintf(v / s) + (float)zp;
  return (int)fminf(fmaxf(q, (float)(off - 128)), (float)(off + 127)) - off;
}

template <int BM, int BN>
__global__ void __launch_bounds__(256) qgemm_kernel(QGemmArgs a) {
  constexpr int LDS_ROW = QG_BK + QG_PAD;
  constexpr int FM = BM / 32, FN = BN / 32;
  constexpr int OUT_ROW = BN + 16;  // staged byte tile: BM x OUT_ROW <= one A buffer
  static_assert(BM * OUT_ROW <= BM * LDS_ROW, "the output tile is staged in an A buffer");
  __shared__ __attribute__((aligned(16))) int8_t sA[2][BM * LDS_ROW];
  __shared__ __attribute__((aligned(16))) int8_t sB[2][BN * LDS_ROW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int M = a.m_ptr ? min(*a.m_ptr, a.M) : a.M;
  const int row0 = blockIdx.y * BM, col0 = blockIdx.x * BN;
  if (row0 >= M) return;
  const int K = a.K, k_pad = a.ldw;
  const int n_kt = (K + QG_BK - 1) / QG_BK;
  const bool xvec = aligned16(a.X, a.ldx);

  constexpr int A_CHUNKS = BM * QG_BK / 16 / 256;
  constexpr int B_CHUNKS = BN * QG_BK / 16 / 256;
  uint4 ra[A_CHUNKS], rb[B_CHUNKS];

  auto load_tile = [&](int kt) {
    const int k0 = kt * QG_BK;
#pragma unroll
    for (int c = 0; c < A_CHUNKS; ++c) {
      const int ch = tid + c * 256;
      const int r = ch >> 3, k = k0 + (ch & 7) * 16;
      const int row = row0 + r;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (row < M && k < K) {
        const int8_t* src = a.X + (size_t)row * a.ldx + k;
        if (xvec && k + 16 <= a.ldx) {
          // bytes between K and ldx are inside the row and meet zero weights
          v = *reinterpret_cast<const uint4*>(src);
        } else {
          uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (k + j < K) w[j >> 2] |= (uint32_t)(uint8_t)src[j] << (8 * (j & 3));
          v = make_uint4(w[0], w[1], w[2], w[3]);
        }
      }
      ra[c] = v;
    }
#pragma unroll
    for (int c = 0; c < B_CHUNKS; ++c) {
      const int ch = tid + c * 256;
      const int r = ch >> 3, k = k0 + (ch & 7) * 16;
      // W is zero padded to [N_pad][K_pad], N_pad a multiple of 128, K_pad of 64
      rb[c] = (k < k_pad) ? *reinterpret_cast<const uint4*>(a.W + (size_t)(col0 + r) * k_pad + k) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int c = 0; c < A_CHUNKS; ++c) {
      const int ch = tid + c * 256;
      *reinterpret_cast<uint4*>(&sA[buf][(ch >> 3) * LDS_ROW + (ch & 7) * 16]) = ra[c];
    }
#pragma unroll
    for (int c = 0; c < B_CHUNKS; ++c) {
      const int ch = tid + c * 256;
      *reinterpret_cast<uint4*>(&sB[buf][(ch >> 3) * LDS_ROW + (ch & 7) * 16]) = rb[c];
    }
  };

  i32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int kt = 0; kt < n_kt; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < n_kt) load_tile(kt + 1);  // global loads in flight under the MFMAs
#pragma unroll
    for (int kk = 0; kk < QG_BK / 64; ++kk) {
      if (kt * QG_BK + kk * 64 >= K) break;  // block-uniform: the second half of a short last tile is all zero
      i32x4 fa[FM], fb[FN];
      const int kof = kk * 64 + 16 * (lane >> 4);
#pragma unroll
      for (int i = 0; i < FM; ++i)
        fa[i] = *reinterpret_cast<const i32x4*>(&sA[cur][(wm * (BM / 2) + i * 16 + (lane & 15)) * LDS_ROW + kof]);
#pragma unroll
      for (int j = 0; j < FN; ++j)
        fb[j] = *reinterpret_cast<const i32x4*>(&sB[cur][(wn * (BN / 2) + j * 16 + (lane & 15)) * LDS_ROW + kof]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < n_kt) store_tile(cur ^ 1);
    __syncthreads();
  }

  // epilogue. The loop ended on a barrier, so buffer 0 of A is free for the staged byte tile.
  int8_t* const sOut = sA[0];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int lc = wn * (BN / 2) + j * 16 + (lane & 15);
      const int col = col0 + lc;
      if (col >= a.N) continue;
      const int corr = a.corr[col];
      const float mult = a.mult[col];
      const float b = a.bias ? a.bias[col] : 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int lr = wm * (BM / 2) + i * 16 + (lane >> 4) * 4 + q;
        const int row = row0 + lr;
        if (row >= M) continue;
        const float v = act_fn((float)(acc[i][j][q] + corr) * mult + b, a.act);
        if (a.y_kind == QY_F32) reinterpret_cast<float*>(a.Y)[(size_t)row * a.ldy + col] = v;
        else if (a.y_kind == QY_BF16) reinterpret_cast<uint16_t*>(a.Y)[(size_t)row * a.ldy + col] = f32_to_bf16(v);
        else sOut[lr * OUT_ROW + lc] = (int8_t)quant_byte(v, a.y_scale, a.y_zp, a.y_off);
      }
    }
  if (a.y_kind != QY_Q8) return;  // kernel-uniform
  __syncthreads();
  // staged tile -> global: 16-byte stores for whole chunks of aligned rows, else dwords, else the live bytes
  int8_t* const Y = reinterpret_cast<int8_t*>(a.Y);
  const bool yvec = aligned16(Y, a.ldy);
  const bool ydw = ((reinterpret_cast<uintptr_t>(Y) | (uintptr_t)(unsigned)a.ldy) & 3) == 0;
  constexpr int OCH = BN / 16;
  for (int ch = tid; ch < BM * OCH; ch += 256) {
    const int lr = ch / OCH, lc = (ch % OCH) * 16;
    const int row = row0 + lr, col = col0 + lc;
    if (row >= M || col >= a.N) continue;
    const int8_t* s = &sOut[lr * OUT_ROW + lc];
    int8_t* d = Y + (size_t)row * a.ldy + col;
    if (yvec && col + 16 <= a.N) {
      *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
      continue;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (ydw && col + 4 * g + 4 <= a.N) {
        *reinterpret_cast<uint32_t*>(d + 4 * g) = *reinterpret_cast<const uint32_t*>(s + 4 * g);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (col + 4 * g + j < a.N) d[4 * g + j] = s[4 * g + j];
      }
    }
  }
}

// QuantizeLinear / DequantizeLinear on one [M][N] tensor with per-tensor parameters: one thread
// per 4 consecutive elements of a row (row_act_kernel's mapping), one pass.
__global__ void __launch_bounds__(256) quant_rows_kernel(QuantRowsArgs a) {
  const int M = a.m_ptr ? min(*a.m_ptr, a.M) : a.M;
  const int N = a.N;
  const int chunks = (N + 3) >> 2;
  const long e = long(blockIdx.x) * 256 + threadIdx.x;
  const int r = int(e / chunks), c0 = int(e - long(r) * chunks) * 4;
  if (r >= M) return;
  const int live = min(4, N - c0);
  if (!a.dequant) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.f_bf16) {
      const uint16_t* x = reinterpret_cast<const uint16_t*>(a.F) + (size_t)r * a.ldf + c0;
      for (int j = 0; j < live; ++j) v[j] = bf16_to_f32(x[j]);
    } else {
      const float* x = reinterpret_cast<const float*>(a.F) + (size_t)r * a.ldf + c0;
      if (live == 4 && aligned16(a.F, a.ldf * 4)) {
        const float4 p = *reinterpret_cast<const float4*>(x);
        v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = p.w;
      } else {
        for (int j = 0; j < live; ++j) v[j] = x[j];
      }
    }
    int8_t* y = a.Q + (size_t)r * a.ldq + c0;
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) w |= (uint32_t)(uint8_t)quant_byte(v[j], a.scale, a.zp, a.off) << (8 * j);
    if (live == 4 && ((reinterpret_cast<uintptr_t>(a.Q) | (uintptr_t)(unsigned)a.ldq) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(y) = w;
    } else {
      for (int j = 0; j < live; ++j) y[j] = (int8_t)(w >> (8 * j));
    }
  } else {
    const int8_t* x = a.Q + (size_t)r * a.ldq + c0;
    for (int j = 0; j < live; ++j) {
      // (q - z) is an exact small integer: one rounding, in the product
      const float v = (float)((int)x[j] + a.off - a.zp) * a.scale;
      if (a.f_bf16) reinterpret_cast<uint16_t*>(a.F)[(size_t)r * a.ldf + c0 + j] = f32_to_bf16(v);
      else reinterpret_cast<float*>(a.F)[(size_t)r * a.ldf + c0 + j] = v;
    }
  }
}

// tile of a launch: 128 x 128 for large batches of wide layers (as launch_gemm), else 64 x 64
int qgemm_tile(int M, int N) { return (M >= 4096 && N >= 128) ? 128 : 64; }

void launch_qgemm(const QGemmArgs& a, hipStream_t st) {
  if (a.M <= 0 || a.N <= 0) return;
  if (qgemm_tile(a.M, a.N) == 128) {
    IGP_LAUNCH((qgemm_kernel<128, 128>), dim3((a.N + 127) / 128, (a.M + 127) / 128), dim3(256), 0, st, a);
  } else {
    IGP_LAUNCH((qgemm_kernel<64, 64>), dim3((a.N + 63) / 64, (a.M + 63) / 64), dim3(256), 0, st, a);
  }
}

void launch_quant_rows(const QuantRowsArgs& a, hipStream_t st) {
  if (a.M <= 0 || a.N <= 0) return;
  const long n = long(a.M) * ((a.N + 3) / 4);
  IGP_LAUNCH(quant_rows_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace igp
