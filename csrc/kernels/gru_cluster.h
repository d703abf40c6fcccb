// What the weight-stationary GRU cluster kernels (gru_ws.hip, gru_wsx.hip) share around their
// recurrence: the rcp-form gate, the stationary-fragment loader, the layer-1 input source kept in
// LDS, and the cluster hand-off protocol (bounded counter waits with poisoning, the NaN pre-fill,
// the final arrival). The kernels keep their MFMA loops, LDS images and publish / gather.
//
// Template parameters: CL workgroups per cluster, M rows per cluster, TWO: the cluster's second
// counter cnt[8] is in use (gru_ws.hip: the launch before may have been the two-half pipeline), so
// a wait that gives up poisons cnt[0] and cnt[8]; otherwise cnt[0] only.
#pragma once
#include "common.h"
#include "launch.h"
#include "seq_input.h"

namespace igp {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int kClusterH = 256;                    // hidden size of every cluster kernel
constexpr uint64_t kClusterWaitTicks = 20000000;  // 200 ms of wall_clock64 (100 MHz): never hang the GPU
constexpr int kSC1 = 16;                          // buffer aux bit: sc1 (L2-coherent, bypasses L1)

// v_exp_f32 + v_rcp_f32 (1 ulp): the IEEE divide sequence of gru.hip's sig_ / tanh_ would cost ~10
// VALU per gate (24 divides per lane per step were as long as a split step's MFMAs,
// tools/gru_wsx_trace.py). Not interchangeable with them: the results differ.
__device__ __forceinline__ float sig_rcp(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_rcp(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * x) + 1.f); }

// bias [6H] (Wb z,r,h | Rb z,r,h) of hidden unit j -> the four gate constants (linear_before_reset = 1)
__device__ __forceinline__ void cluster_bias(const float* bs, int H, int j, float (&bv)[4]) {
  bv[0] = bs[j] + bs[3 * H + j];
  bv[1] = bs[H + j] + bs[4 * H + j];
  bv[2] = bs[2 * H + j];
  bv[3] = bs[5 * H + j];
}

// one element's gates from its four sums (z, r, input half of h~, recurrent half of h~) -> new h
__device__ __forceinline__ float cluster_gate(float az, float ar, float ax, float ah, const float (&bv)[4], float h) {
  const float z = sig_rcp(az + bv[0]);
  const float rr = sig_rcp(ar + bv[1]);
  const float hh = tanh_rcp(ax + bv[2] + rr * (ah + bv[3]));
  return (1.f - z) * hh + z * h;
}

// packed fragment (nt, ks) of a [N/16][KS][64][8] bf16 weight (ops/kernels.py pack_fragments)
__device__ __forceinline__ bf16x8 cluster_wfrag(const uint16_t* p, int nt, int KS, int ks, int lane) {
  const uint4 v = *reinterpret_cast<const uint4*>(p + (((size_t)nt * KS + ks) * 64 + lane) * 8);
  return __builtin_bit_cast(bf16x8, v);
}

// ---- layer-1 input: chunk c = (row c / chunks, 8-element piece c % chunks). Every chunk's source
// goes to LDS once (xmeta[c], seq_src_pack), and only the layer-1 waves stage x_{t+1} from it.
template <int M>
__device__ __forceinline__ void cluster_x_sources(const GruArgs& a, int2* xmeta, int row0, int n_live, int chunks,
                                                  int tid) {
  for (int c = tid; c < M * chunks; c += 256) xmeta[c] = seq_src_pack(seq_src(a, row0 + c / chunks, n_live));
}

__device__ __forceinline__ uint4 cluster_load_x(const GruArgs& a, const int2* xmeta, int row0, int chunks, int c, int t) {
  const SeqSrc s = seq_src_unpack(xmeta[c]);
  const int row = c / chunks;
  return seq_load(a, s, row0 + row, c - row * chunks, t);
}

__device__ __forceinline__ void cluster_load_x_split(const GruArgs& a, const int2* xmeta, int row0, int chunks, int c,
                                                     int t, uint4& hi, uint4& lo) {
  const SeqSrc s = seq_src_unpack(xmeta[c]);
  const int row = c / chunks;
  seq_load_split(a, s, row0 + row, c - row * chunks, t, hi, lo);
}

// Outputs start as NaN: a cluster that gives up (bounded wait) leaves them so, and the host
// detects it (AbuseGpu.wait) instead of reading the previous batch's values. UW: hidden units per member.
template <int M, int UW>
__device__ __forceinline__ void cluster_nan_fill(const GruArgs& a, int row0, int n_live, int mem, int tid) {
  if (a.head_w && mem == 0 && tid < M && row0 + tid < n_live) a.out[row0 + tid] = __builtin_nanf("");
  if (a.yh)
    for (int e = tid; e < M * UW; e += 256) {
      const int row = row0 + e / UW;
      if (row < n_live) a.yh[(size_t)row * kClusterH + mem * UW + e % UW] = __builtin_nanf("");
    }
}

// Bounded poll of a cluster counter by one lane; returns false on timeout, after poisoning the
// cluster's counters (`base`, launch.h kClusterPoison) so that no member still to arrive and no
// launch queued behind this one passes a wait on a part-advanced count.
template <bool TWO>
__device__ __forceinline__ bool cluster_wait(int32_t* cnt, int target, int32_t* base) {
  const uint64_t t0 = wall_clock64();
  for (;;) {
    for (int n = 0; n < 64; ++n) {
      if (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) return true;
      __builtin_amdgcn_s_sleep(1);
    }
    if (wall_clock64() - t0 > kClusterWaitTicks) {
      __hip_atomic_exchange(base, kClusterPoison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (TWO) __hip_atomic_exchange(base + 8, kClusterPoison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
  }
}

// One lane arrives at `cnt` (if `arrive`) and waits for `target` (if `wait`); the outcome goes to
// every wave through *sflag. False: the wait gave up, *a.ws_err is set and the workgroup must exit.
// CONTAINS A __syncthreads(): call it from all waves of the workgroup.
template <bool TWO>
__device__ __forceinline__ bool cluster_arrive_wait(const GruArgs& a, int32_t* cnt, int target, int32_t* base,
                                                    bool arrive, bool wait, int* sflag, int tid) {
  if (tid == 0) {
    if (arrive) __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool ok = true;
    if (wait) {
      ok = cluster_wait<TWO>(cnt, target, base);
      if (!ok) atomicExch(a.ws_err, 1);
    }
    *sflag = ok;
  }
  __syncthreads();
  return *sflag != 0;
}

// h_{T-1} of this lane's hidden unit j (RT row tiles, accumulator layout) -> yh, and its head
// products summed over the tile's 16 lanes -> red[row] (one f32 per row and hidden tile).
template <int RT>
__device__ __forceinline__ void cluster_emit(const GruArgs& a, const float (&hs)[RT][4], int row0, int n_live, int j,
                                             int crow, int ccol, float* red) {
  if (a.yh) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + rt * 16 + crow + r;
        if (row < n_live) a.yh[(size_t)row * kClusterH + j] = hs[rt][r];
      }
  }
  if (a.head_w) {
    const float w = a.head_w[j];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = hs[rt][r] * w;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
        if (ccol == 0) red[rt * 16 + crow + r] = v;
      }
  }
}

// The end of a launch, after the barrier that completes red[NRED][M] (this member's head partials
// per hidden tile): the member's partial goes to the workspace, every member arrives a last time,
// member 0 waits for all CL, sums the partials in member order (deterministic), applies the head
// activation and returns the counter(s) to 0. The reset must take the atomic path: a memset node
// between graph replays left a stale counter line visible to the next replay's sc1 polls.
// RESET2: cnt[8] advanced in this launch as well (the two-half pipeline).
// CONTAINS TWO __syncthreads(): call it from all waves of the workgroup.
template <int CL, int M, int NRED, bool TWO, bool RESET2>
__device__ __forceinline__ void cluster_finish(const GruArgs& a, int32_t* cnt, int cl, int mem, int row0, int n_live,
                                               const float* red, int* sflag, int tid) {
  float* const part = a.ws_part + (size_t)cl * CL * M;
  if (a.head_w && tid < M) {
    float v = red[tid];
#pragma unroll
    for (int k = 1; k < NRED; ++k) v += red[k * M + tid];
    __hip_atomic_store(part + mem * M + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const bool ok = cluster_arrive_wait<TWO>(a, cnt, CL * (a.T + 1), cnt, true, mem == 0, sflag, tid);
  if (mem != 0 || !ok) return;
  if (a.head_w && tid < M && row0 + tid < n_live) {
    float v = a.head_b;
#pragma unroll
    for (int m2 = 0; m2 < CL; ++m2)
      v += __hip_atomic_load(part + m2 * M + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.head_act == 2) v = 1.f / (1.f + expf(-v));
    a.out[row0 + tid] = v;
  }
  if (tid == 0) {
    __hip_atomic_exchange(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (RESET2) __hip_atomic_exchange(cnt + 8, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace igp
