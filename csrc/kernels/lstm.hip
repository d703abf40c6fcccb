// K4 (LSTM): stacked ONNX LSTM (1-2 layers, gates i, o, f, c, sigmoid / tanh / tanh, zero initial
// states) over a per-account event history, with the N=1 head (Gemm + Sigmoid) fused.
//
// The batch-parallel design of gru.hip: a workgroup owns M = 16*RT sequences and runs ALL T steps
// of BOTH layers for them, so there is no grid-wide synchronisation. Per step and layer:
//   gates[M, 4H] = x_t[M, K] . W^T  +  h_{t-1}[M, H] . R^T        (MFMA 16x16x32 bf16)
//   c = f * c + i * c~ ;  h = o * tanh(c)
// All four gates take both products, so a layer step is ONE pass and one block barrier (the GRU's
// linear_before_reset = 0 second pass and its r*h buffer have no counterpart here). Weights stream
// from L2 as fragment-packed 1 KiB wave loads through a buffer resource; x_t / h_{t-1}
// A-fragments come from LDS (bf16, ping-pong per layer). The f32 hidden state h AND the f32 cell
// state c stay in registers: lane (l&15, l>>4) of the wave that owns hidden tile ht computes the
// same (row, unit) every step, so the gates combine lane-locally and c never reaches LDS or HBM.
//
// SPLIT = 1 (fp32 plans): weights and activations are bf16 pairs hi + lo, each product three
// MFMAs (lo*hi + hi*lo + hi*hi) into f32 accumulators, activation tiles doubled in LDS.
// SPLIT = 0 (bf16 plans): one MFMA per product.
// The layer-1 input staging is seq_input.h's, shared with gru.hip and the cluster kernels.
#include "common.h"
#include "launch.h"
#include "seq_input.h"
#include "seq_window.h"

namespace igp {

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int LSTM_PAD = 8;  // bf16 row padding in LDS (16 B)

__device__ __forceinline__ float sig_(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_(float x) { return 1.f - 2.f / (__expf(2.f * x) + 1.f); }

// Weight fragments through a buffer resource: one VGPR (lane*16) is the per-lane part of every
// fragment load, the fragment index goes into the scalar offset.
struct WFrag {
  __amdgpu_buffer_rsrc_t rsrc;
  int voff;
};

__device__ __forceinline__ WFrag wfrag(const uint16_t* base, size_t elems, int lane) {
  WFrag w;
  w.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(base), 0, (int)(elems * 2), 0x00020000);
  w.voff = lane * 16;
  return w;
}

__device__ __forceinline__ bf16x8 ld_frag(const WFrag& w, int nt, int KS, int ks) {
  const int soff = __builtin_amdgcn_readfirstlane((nt * KS + ks) * 1024);
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(w.rsrc, w.voff, soff, 0);
  return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ bf16x8 lds_frag(const uint16_t* base, int stride, int row, int k) {
  const uint4 v = *reinterpret_cast<const uint4*>(base + row * stride + k);
  return *reinterpret_cast<const bf16x8*>(&v);
}

// acc += a . b: one MFMA, or the three of the hi / lo split (lo*lo ~2^-18 relative is dropped)
template <int SPLIT>
__device__ __forceinline__ void mma(f32x4& acc, const bf16x8& ah, const bf16x8& al, const bf16x8& bh,
                                    const bf16x8& bl) {
  if constexpr (SPLIT != 0) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
  }
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
}

struct WPair {  // a weight matrix as hi (and, split, lo) fragment streams
  WFrag hi, lo;
};

// acc[gate][rt] += act[M, KS*32] . Wg^T for the four gate tiles of hidden tile ht
template <int RT, int KS, int HT, int SPLIT>
__device__ __forceinline__ void gate_products(f32x4 (&acc)[4][RT], const WPair& w, const uint16_t* act,
                                              const uint16_t* actl, int stride, int ht, int arow, int akof) {
#pragma unroll 2
  for (int ks = 0; ks < KS; ++ks) {
    bf16x8 b[4], bl[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      b[g] = ld_frag(w.hi, g * HT + ht, KS, ks);
      if constexpr (SPLIT != 0) bl[g] = ld_frag(w.lo, g * HT + ht, KS, ks);
      else bl[g] = b[g];
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const bf16x8 a = lds_frag(act, stride, rt * 16 + arow, ks * 32 + akof);
      bf16x8 al = a;
      if constexpr (SPLIT != 0) al = lds_frag(actl, stride, rt * 16 + arow, ks * 32 + akof);
#pragma unroll
      for (int g = 0; g < 4; ++g) mma<SPLIT>(acc[g][rt], a, al, b[g], bl[g]);
    }
  }
}

// One LSTM layer step for this wave's hidden tiles. KSI / KSH: K/32 of the input / hidden parts;
// bias: [4H] with Wb + Rb already summed per gate.
// MASKED: live(rt, r) says whether accumulator row rt*16 + crow + r is inside its window at this
// step; a dead row keeps h and c and carries h's bf16 (hi / lo) value into hnext.
template <int RT, int KSI, int KSH, int NW, int SPLIT, int MASKED = 0>
__device__ __forceinline__ void lstm_step(const WPair& gW, const WPair& gR, const float* bias, const uint16_t* in,
                                          const uint16_t* inl, int in_stride, const uint16_t* hprev,
                                          const uint16_t* hprevl, uint16_t* hnext, uint16_t* hnextl,
                                          float (&hs)[KSH * 2 / NW][RT][4], float (&cs)[KSH * 2 / NW][RT][4],
                                          int lane, int wave, const SeqLive<MASKED>& live) {
  constexpr int HT = KSH * 2;      // hidden tiles of 16 units
  constexpr int HTW = HT / NW;     // per wave
  constexpr int H = KSH * 32;
  constexpr int HS = H + LSTM_PAD;
  const int arow = lane & 15, akof = 8 * (lane >> 4);
  const int crow = (lane >> 4) * 4, ccol = lane & 15;
#pragma unroll
  for (int i = 0; i < HTW; ++i) {
    const int ht = wave + NW * i;
    f32x4 acc[4][RT];  // i, o, f, c~
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[g][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    gate_products<RT, KSI, HT, SPLIT>(acc, gW, in, inl, in_stride, ht, arow, akof);
    gate_products<RT, KSH, HT, SPLIT>(acc, gR, hprev, hprevl, HS, ht, arow, akof);
    const int j = ht * 16 + ccol;
    const float bi = bias[j], bo = bias[H + j], bf = bias[2 * H + j], bc = bias[3 * H + j];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ig = sig_(acc[0][rt][r] + bi);
        const float og = sig_(acc[1][rt][r] + bo);
        const float fg = sig_(acc[2][rt][r] + bf);
        const float ct = tanh_(acc[3][rt][r] + bc);
        float c = fg * cs[i][rt][r] + ig * ct;
        float h = og * tanh_(c);
        if constexpr (MASKED != 0) {
          const bool on = live(rt, r);
          c = on ? c : cs[i][rt][r];
          h = on ? h : hs[i][rt][r];
        }
        cs[i][rt][r] = c;
        hs[i][rt][r] = h;
        const int o = (rt * 16 + crow + r) * HS + j;
        if constexpr (SPLIT != 0) bf16_split(h, hnext[o], hnextl[o]);
        else hnext[o] = f32_to_bf16(h);
      }
  }
}

template <int RT, int KSH, int NW>
__device__ __forceinline__ void emit_outputs(const LstmArgs& a, float (&hs)[KSH * 2 / NW][RT][4], float* red,
                                             int row0, int n_live, int lane, int wave, int tid) {
  constexpr int M = RT * 16, H = KSH * 32, HTW = KSH * 2 / NW;
  const int crow = (lane >> 4) * 4, ccol = lane & 15;
  if (a.yh) {
#pragma unroll
    for (int i = 0; i < HTW; ++i)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + rt * 16 + crow + r;
          if (row < n_live) a.yh[(size_t)row * H + (wave + NW * i) * 16 + ccol] = hs[i][rt][r];
        }
  }
  if (a.head_w) {
    float part[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[rt][r] = 0.f;
#pragma unroll
    for (int i = 0; i < HTW; ++i) {
      const float w = a.head_w[(wave + NW * i) * 16 + ccol];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[rt][r] += hs[i][rt][r] * w;
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = part[rt][r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
        if (ccol == 0) red[wave * M + rt * 16 + crow + r] = v;
      }
    __syncthreads();
    if (tid < M && row0 + tid < n_live) {
      float v = a.head_b;
#pragma unroll
      for (int w = 0; w < NW; ++w) v += red[w * M + tid];
      if (a.head_act == 2) v = 1.f / (1.f + expf(-v));
      a.out[row0 + tid] = v;
    }
  }
}

// MASKED: per-row sequence lengths. The my_c == 0 stager of each row publishes the row's live
// window in LDS (wl[M], after red); every step each lane tests the windows of its accumulator
// rows (SeqLive). Dead steps skip nothing: the barriers stay block-uniform.
template <int RT, int KSX, int KSH, int NW, int SPLIT, int MASKED = 0>
__global__ void __launch_bounds__(NW * 64) lstm_kernel(LstmArgs a) {
  constexpr int M = RT * 16;
  constexpr int H = KSH * 32;
  constexpr int HS = H + LSTM_PAD;
  constexpr int XS = KSX * 32 + LSTM_PAD;
  constexpr int HTW = KSH * 2 / NW;
  constexpr int NT = NW * 64;
  constexpr int NH = SPLIT ? 2 : 1;  // activation halves in LDS (hi | lo)
  static_assert(KSH * 2 % NW == 0, "hidden tiles must divide over the waves");
  static_assert(M * (KSX * 4) <= NT, "one staging thread per (row, 8-element chunk)");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_live = a.m_ptr ? min(*a.m_ptr, a.n_rows) : a.n_rows;
  const int row0 = blockIdx.x * M;
  if (row0 >= n_live) return;  // block-uniform: no barrier is left waiting
  const size_t wx = (size_t)4 * H * KSX * 32, wh = (size_t)4 * H * H;
  const bool two = a.n_layers == 2;
  const int l1 = two ? 1 : 0;  // a one-layer model never runs layer 2: its streams alias layer 1's
  WPair w0, r0, w1, r1;
  w0.hi = wfrag(a.layer[0].W, wx, lane);
  r0.hi = wfrag(a.layer[0].R, wh, lane);
  w1.hi = wfrag(a.layer[l1].W, two ? wh : wx, lane);
  r1.hi = wfrag(a.layer[l1].R, wh, lane);
  if constexpr (SPLIT != 0) {
    w0.lo = wfrag(a.layer[0].W_lo, wx, lane);
    r0.lo = wfrag(a.layer[0].R_lo, wh, lane);
    w1.lo = wfrag(a.layer[l1].W_lo, two ? wh : wx, lane);
    r1.lo = wfrag(a.layer[l1].R_lo, wh, lane);
  } else {
    w0.lo = w0.hi; r0.lo = r0.hi; w1.lo = w1.hi; r1.lo = r1.hi;
  }

  // ---- LDS: hb[NH halves][layer][pingpong][M][HS] | xb[NH halves][pingpong][M][XS] | bias[2][4H] | red[NW][M]
  uint16_t* const hb = reinterpret_cast<uint16_t*>(smem);
  uint16_t* const xb = hb + NH * 4 * M * HS;
  float* const bias = reinterpret_cast<float*>(xb + NH * 2 * M * XS);
  float* const red = bias + 8 * H;
#define HB(half, l, b) (hb + ((half) * 4 + (l) * 2 + (b)) * (M * HS))
#define XB(half, b) (xb + ((half) * 2 + (b)) * (M * XS))
  // zero h_0 (both layers, both buffers) and the x buffers (their K padding stays zero)
  {
    uint32_t* z = reinterpret_cast<uint32_t*>(smem);
    const int words = NH * (4 * M * HS + 2 * M * XS) / 2;
    for (int i = tid; i < words; i += NT) z[i] = 0u;
  }
  for (int i = tid; i < 4 * H; i += NT) {  // Wb + Rb per gate
    bias[i] = a.layer[0].bias[i] + a.layer[0].bias[4 * H + i];
    bias[4 * H + i] = two ? a.layer[1].bias[i] + a.layer[1].bias[4 * H + i] : 0.f;
  }

  // ---- layer-1 input staging: thread -> (row rr, 8-element chunk c), fixed for all t
  const int chunks = a.I >> 3;
  const int my_rr = tid / max(chunks, 1), my_c = tid - my_rr * max(chunks, 1);
  const bool stager = chunks > 0 && my_rr < M;
  const int grow = row0 + my_rr;
  const SeqSrc src = stager ? seq_src(a, grow, n_live) : SeqSrc{-1, 0, a.T};
  // x_t as (hi, lo) bf16 halves; a bf16 (SPLIT = 0) kernel never stores lo
  auto load_x = [&](int t, uint4& hi, uint4& lo) {
    if constexpr (SPLIT != 0) seq_load_split(a, src, grow, my_c, t, hi, lo);
    else hi = seq_load(a, src, grow, my_c, t);
  };
  auto store_x = [&](int b, const uint4& hi, const uint4& lo) {
    *reinterpret_cast<uint4*>(XB(0, b) + my_rr * XS + my_c * 8) = hi;
    if constexpr (SPLIT != 0) *reinterpret_cast<uint4*>(XB(1, b) + my_rr * XS + my_c * 8) = lo;
  };
  if constexpr (MASKED != 0) {
    if (stager && my_c == 0) reinterpret_cast<uint32_t*>(red + NW * M)[my_rr] = seq_window(a, grow, n_live, src.from);
  }
  __syncthreads();  // zeroing done before the first staged row lands
  if (stager) {
    uint4 h, l;
    load_x(0, h, l);
    store_x(0, h, l);
  }
  float hs0[HTW][RT][4], cs0[HTW][RT][4], hs1[HTW][RT][4], cs1[HTW][RT][4];
#pragma unroll
  for (int i = 0; i < HTW; ++i)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) hs0[i][rt][r] = cs0[i][rt][r] = hs1[i][rt][r] = cs1[i][rt][r] = 0.f;
  __syncthreads();

  // the lo halves of a bf16 (SPLIT = 0) kernel are never read: they alias the hi halves
  constexpr int LO = SPLIT ? 1 : 0;
  for (int t = 0; t < a.T; ++t) {
    const int pb = t & 1, nb = pb ^ 1;
    SeqLive<MASKED> live;
    if constexpr (MASKED != 0)
      live = {reinterpret_cast<const uint32_t*>(red + NW * M), (lane >> 4) * 4, a.reverse ? a.T - 1 - t : t};
    uint4 xh, xl;
    load_x(t + 1, xh, xl);
    lstm_step<RT, KSX, KSH, NW, SPLIT, MASKED>(w0, r0, bias, XB(0, pb), XB(LO, pb), XS, HB(0, 0, pb), HB(LO, 0, pb),
                                               HB(0, 0, nb), HB(LO, 0, nb), hs0, cs0, lane, wave, live);
    __syncthreads();
    if (two) {
      lstm_step<RT, KSH, KSH, NW, SPLIT, MASKED>(w1, r1, bias + 4 * H, HB(0, 0, nb), HB(LO, 0, nb), HS, HB(0, 1, pb),
                                                 HB(LO, 1, pb), HB(0, 1, nb), HB(LO, 1, nb), hs1, cs1, lane, wave,
                                                 live);
    }
    if (stager && t + 1 < a.T) store_x(nb, xh, xl);
    __syncthreads();
  }

  // ---- outputs from the last layer's registers (static register indexing in both branches)
  if (two)
    emit_outputs<RT, KSH, NW>(a, hs1, red, row0, n_live, lane, wave, tid);
  else
    emit_outputs<RT, KSH, NW>(a, hs0, red, row0, n_live, lane, wave, tid);
#undef HB
#undef XB
}

// masked: the M window words after red
size_t lstm_lds_bytes(int RT, int KSX, int KSH, int NW, int split, int masked = 0) {
  const int M = RT * 16, H = KSH * 32, HS = H + LSTM_PAD, XS = KSX * 32 + LSTM_PAD, NH = split ? 2 : 1;
  return (size_t)NH * (4 * M * HS + 2 * M * XS) * 2 + (size_t)2 * 4 * H * 4 + (size_t)NW * M * 4 +
         (masked ? (size_t)M * 4 : 0);
}

constexpr size_t kLdsLimit = 160 * 1024;

// waves per workgroup: two hidden tiles per wave from H = 128 up (as the GRU kernels), one at H = 64
constexpr int lstm_waves(int KSH) { return KSH >= 4 ? 8 : 4; }

// The 32-row choice is made on the unmasked footprint (lstm_tile_rows), so a masked launch takes
// the same tile as its unmasked twin; the window words must then fit too.
template <int KSX, int KSH, int SPLIT, int MASKED>
void launch_lstm_t(const LstmArgs& a, hipStream_t st) {
  constexpr int NW = lstm_waves(KSH);
  const dim3 block(NW * 64);
  // 32 rows per workgroup feed every streamed weight fragment to two row tiles; only on request
  // (tile_rows = 32) and only where the doubled activation tiles stay within the LDS
  if (a.tile_rows == 32 && lstm_lds_bytes(2, KSX, KSH, NW, SPLIT) <= kLdsLimit &&
      lstm_lds_bytes(2, KSX, KSH, NW, SPLIT, MASKED) <= kLdsLimit) {
    IGP_LAUNCH((lstm_kernel<2, KSX, KSH, NW, SPLIT, MASKED>), dim3((a.n_rows + 31) / 32), block,
               lstm_lds_bytes(2, KSX, KSH, NW, SPLIT, MASKED), st, a);
    return;
  }
  IGP_LAUNCH((lstm_kernel<1, KSX, KSH, NW, SPLIT, MASKED>), dim3((a.n_rows + 15) / 16), block,
             lstm_lds_bytes(1, KSX, KSH, NW, SPLIT, MASKED), st, a);
}

template <int KSX, int KSH, int MASKED>
void launch_lstm_s(const LstmArgs& a, hipStream_t st) {
  if (a.split) launch_lstm_t<KSX, KSH, 1, MASKED>(a, st);
  else launch_lstm_t<KSX, KSH, 0, MASKED>(a, st);
}

template <int KSH, int MASKED>
void launch_lstm_h(const LstmArgs& a, hipStream_t st) {
  if (a.layer[0].kx_pad == 32) launch_lstm_s<1, KSH, MASKED>(a, st);
  else launch_lstm_s<2, KSH, MASKED>(a, st);
}

template <int MASKED>
void launch_lstm_m(const LstmArgs& a, hipStream_t st) {
  switch (a.H) {
    case 64: launch_lstm_h<2, MASKED>(a, st); break;
    case 128: launch_lstm_h<4, MASKED>(a, st); break;
    case 256: launch_lstm_h<8, MASKED>(a, st); break;
    default: break;
  }
}

}  // namespace

#ifdef IGP_LSTM_MASKED_TU
// lstm_masked.hip: this file again, for the MASKED = 1 instances alone
void launch_lstm_masked(const LstmArgs& a, hipStream_t st) { launch_lstm_m<1>(a, st); }
#else
int lstm_tile_rows(int H, int kx_pad, int split, int requested) {
  const int KSH = H / 32;
  return requested == 32 && lstm_lds_bytes(2, kx_pad / 32, KSH, lstm_waves(KSH), split) <= kLdsLimit ? 32 : 16;
}

void launch_lstm(const LstmArgs& a, hipStream_t st) {
  if (a.n_rows <= 0) return;
  if (a.masked) return launch_lstm_masked(a, st);
  launch_lstm_m<0>(a, st);
}
#endif

}  // namespace igp
