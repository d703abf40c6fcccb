// Column assembly (models/plan.py ColumnStep): the front end of a scikit-learn ColumnTransformer
// pipeline - impute, scale, one-hot encode, binarise, select - as ONE launch in front of the
// estimator, instead of a diagonal dense layer per Scaler and a join per Concat input.
//
//   Y[r][j] = mode_j(affine_j(impute_j(X[r][src_j])))        j < out_width, r < live rows
//
// with one ColRecord per output column (launch.h): impute x = hit ? value : x (hit = isnan(x), or
// x == replaced), then (x - sub) * mul as an f32 subtract and an f32 multiply (never fused: the
// build sets -ffp-contract=off), then pass | truncf(x) == arg | x > arg | 0. This is the CPU
// executor's arithmetic, so the result is bit-equal to it.
//
// Memory-bound and tiny. A 256-thread workgroup takes COL_TILE_ROWS rows x 256 output columns:
// it stages its X rows (in_width <= COL_MAX_IN columns) and its 256 records in LDS once, 16-byte
// loads where the base and stride allow and element loads otherwise; then lane l of every wave
// keeps the 4 records of columns 4l .. 4l + 3 in registers and the four waves walk the rows, so a
// wave writes one row's 1 KiB run with 16-byte stores (8-byte for a bf16 Y; element stores for the
// row tail and unaligned strides). Nothing is read past in_width or written past out_width, and
// rows at or past the live count (m_ptr) are neither read nor written.
#include "common.h"
#include "launch.h"

namespace igp {

namespace {

static_assert(sizeof(ColRecord) == 32, "ColRecord is two 16-byte words");

__device__ __forceinline__ float col_eval(const ColRecord& r, float x) {
  if (r.flags & COL_IMPUTE) {
    const bool hit = (r.flags & COL_IMP_NAN) ? (x != x) : (x == r.replaced);
    x = hit ? r.value : x;
  }
  if (r.flags & COL_AFFINE) x = (x - r.sub) * r.mul;
  switch (r.flags & COL_MODE_MASK) {
    case COL_ONEHOT: return truncf(x) == r.arg ? 1.f : 0.f;
    case COL_BINARIZE: return x > r.arg ? 1.f : 0.f;
    case COL_ZERO: return 0.f;
    default: return x;
  }
}

__global__ void __launch_bounds__(256) col_assemble_kernel(ColArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[COL_TILE_ROWS * COL_MAX_IN];
  __shared__ __attribute__((aligned(16))) ColRecord recs[256];
  const int M = a.m_ptr ? min(*a.m_ptr, a.M) : a.M;
  const int r0 = blockIdx.x * COL_TILE_ROWS;
  if (r0 >= M) return;  // the whole workgroup
  const int rows = min(COL_TILE_ROWS, M - r0);
  const int tid = threadIdx.x;
  const int W = a.in_width, ldsw = (W + 3) & ~3;

  // this workgroup's records, one per thread (the table is padded to a multiple of 4 columns)
  const int col_base = blockIdx.y * 256;
  if (col_base + tid < ((a.out_width + 3) & ~3)) {
    const int4* s = reinterpret_cast<const int4*>(a.tab + col_base + tid);
    int4* d = reinterpret_cast<int4*>(&recs[tid]);
    d[0] = s[0];
    d[1] = s[1];
  }
  // the X tile: 4-column chunks, consecutive threads on consecutive chunks of a row
  const bool xv = (a.ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(a.X) & 15u) == 0;
  const int chunks = ldsw >> 2;
  for (int e = tid; e < rows * chunks; e += 256) {
    const int rr = e / chunks, c0 = (e - rr * chunks) * 4;
    const float* row = a.X + size_t(r0 + rr) * size_t(a.ldx);
    float4 v;
    if (xv && c0 + 4 <= W) {
      v = *reinterpret_cast<const float4*>(row + c0);
    } else {
      v.x = c0 < W ? row[c0] : 0.f;
      v.y = c0 + 1 < W ? row[c0 + 1] : 0.f;
      v.z = c0 + 2 < W ? row[c0 + 2] : 0.f;
      v.w = c0 + 3 < W ? row[c0 + 3] : 0.f;
    }
    *reinterpret_cast<float4*>(&xs[rr * ldsw + c0]) = v;
  }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6;
  const int c0 = col_base + lane * 4;
  if (c0 >= a.out_width) return;
  ColRecord rc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    rc[k] = recs[lane * 4 + k];
    rc[k].src = min(max(rc[k].src, 0), W - 1);  // the host checked it; a bad table still reads inside the tile
  }
  const int esz = a.y_bf16 ? 2 : 4;
  const bool yv = (a.ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(a.Y) & (a.y_bf16 ? 7u : 15u)) == 0 &&
                  c0 + 4 <= a.out_width;
  for (int rr = wave; rr < rows; rr += 4) {
    const float* x = &xs[rr * ldsw];
    float y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = col_eval(rc[k], x[rc[k].src]);
    char* out = static_cast<char*>(a.Y) + (size_t(r0 + rr) * size_t(a.ldy) + size_t(c0)) * esz;
    if (yv) {
      if (a.y_bf16) {
        uint2 u;
        u.x = uint32_t(f32_to_bf16(y[0])) | (uint32_t(f32_to_bf16(y[1])) << 16);
        u.y = uint32_t(f32_to_bf16(y[2])) | (uint32_t(f32_to_bf16(y[3])) << 16);
        *reinterpret_cast<uint2*>(out) = u;
      } else {
        *reinterpret_cast<float4*>(out) = make_float4(y[0], y[1], y[2], y[3]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + k < a.out_width) {
          if (a.y_bf16) reinterpret_cast<uint16_t*>(out)[k] = f32_to_bf16(y[k]);
          else reinterpret_cast<float*>(out)[k] = y[k];
        }
    }
  }
}

}  // namespace

void launch_col_assemble(const ColArgs& a, hipStream_t st) {
  if (a.M <= 0 || a.out_width <= 0) return;
  const dim3 grid(unsigned((a.M + COL_TILE_ROWS - 1) / COL_TILE_ROWS), unsigned((a.out_width + 255) / 256));
  IGP_LAUNCH(col_assemble_kernel, grid, dim3(256), 0, st, a);
}

}  // namespace igp
