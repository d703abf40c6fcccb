// Kernel argument blocks and host launch entry points of the _hipk extension.
// Every launch takes an explicit hipStream_t (torch's current stream from Python) and
// performs no allocation or synchronisation, so all of them are hipGraph-capturable.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../include/device_ops.h"
#include "../include/records.h"
#include "oplist.h"

namespace igp {

// events of one account per batch held in its dedup list (more: ordered scan of the batch)
constexpr int DEDUP_LIST = 64;
// scorer path, a batch in which no account has more events than this (AssembleArgs::own_short):
// every multi-event account is scored and applied inside K1, led by the quarter-wave of its first
// row (one list entry per lane), and no update_segments launch follows
constexpr int K1_SEG_MAX = 16;
static_assert(K1_SEG_MAX <= DEDUP_LIST, "K1 reads a short account's rows from its dedup list");

// scorer batches rotate over DEDUP_RING dedup regions by BatchHdr::seq: batch q's K1 clears the
// region of batch q + DEDUP_AHEAD (= q - 1's, consumed by then), so batch q+1's dedup insert
// (copy stream) can run while batch q is still in K1 / update_segments on the state stream.
// The copy of batch q waits for the state stage of batch q - DEDUP_AHEAD (the native driver keeps
// one post-state event per ring entry and only queues the wait when the host does not already see
// that batch complete). Eight regions let the pipeline run up to seven batches deep without that
// wait: with four, depth 4 collapsed (r4 NOTES). Region DEDUP_STANDALONE: event ingestion.
constexpr int DEDUP_RING = 8;
constexpr int DEDUP_AHEAD = DEDUP_RING - 1;
constexpr int DEDUP_STANDALONE = DEDUP_RING;
__host__ __device__ inline int dedup_ring_region(int seq) { return (int)((unsigned)seq % DEDUP_RING); }

// Dedup scratch: DEDUP_RING + 1 regions, each = keys/first/count/fill [cap] + list [cap][DEDUP_LIST] + mlist [dmax]
// + 2 counters (update.h dedup_region).
struct UpdateArgs {
  const ScoreCfg* cfg;
  const BatchHdr* hdr;      // scorer path: live count + seq parity (nullable -> n, region)
  int32_t n;
  int32_t n_max;            // grid coverage
  const ReqRec* req;        // events (ReqRec.ts = event time)
  uint32_t* ring_ts;
  int64_t* ring_amt;
  uint8_t* hll;
  AcctRT* rt;
  uint16_t* ev;             // event ring bf16 [C][ev_ring][16] (nullable)
  int32_t ring_size;
  int32_t ev_ring;
  int32_t ev_dim;
  int32_t* dbuf;
  int32_t dcap;             // power of two >= 2 * dmax
  int32_t dmax;
  int32_t region;           // -1: hdr->seq & 1; else fixed region (2 = standalone)
  // scorer dedup insert only (nullable): the pinned host slab [BatchHdr | ReqRec x n]; the kernel
  // reads the batch from it and writes the device copy (hdr, req) for the later stages
  const char* src;
  // with src only (nullable): the slot's segment table in pinned host memory. nseg > 0: the rows
  // are not behind the slab's header but in the host buffers the table names (device_ops.h)
  const IgpRowSegTable* segs;
  const int32_t* hll_lc;   // [257] linear-counting table (the cached HLL estimates, AcctRT)
  // scorer dedup insert of the rows-region exchange only (nullable): the rows come from this
  // owner's chunk of every sender's block of the node-shared rows region (sender p's chunk at
  // xrecv + p * xpstride: header record {slot = count, ts = sender clock} + up to xc rows); the
  // kernel compacts them into req (sender order, then row order), writes route[i] = p * xc + j,
  // route[n_max] = rows over capacity, and the header {n, seq (from xhdr), now}
  const ReqRec* xrecv;
  int32_t* route;
  const int4* xhdr;
  int32_t xn, xc;
  int32_t xpstride;
};

struct AssembleArgs {
  const BatchHdr* hdr;
  const ScoreCfg* cfg;
  const ReqRec* req;        // [n_rows]
  const uint32_t* ring_ts;
  const int64_t* ring_amt;
  const uint8_t* hll;       // [C][2][256]
  const AcctRT* rt;
  const AcctBatch* batch;
  const float* ext;         // [C][ext_width]
  const uint64_t* bl_keys;  // blacklist open-addressing table (nullable)
  const uint32_t* bl_exp;
  const uint64_t* ip_keys;  // ip-intel table (nullable)
  const uint32_t* ip_flags;
  const int32_t* hll_lc;    // [257]: floor(256 ln(256 / v) + 0.5), HLL linear counting by zero count v
  float* X;                 // [n_rows][x_stride]
  FeatRec* feat;            // [n_rows]
  // [n_rows][128 B] D2H image of each row (nullable): the raw FeatRec, or for a request with
  // ReqRec.tx_type bit FV_ENC_BIT the encoded risk.v1 FeatureVector body (features.hip write_fenc)
  uint8_t* fenc;
  // nullable: fenc is routed like EnsembleArgs::route - live row i's image goes to
  // fenc + p * fenc_stride + j * 128 bytes (route[i] = p * fenc_c + j); padding rows write none
  const int32_t* fenc_route;
  int32_t fenc_c;
  int32_t fenc_stride;
  int32_t* dbuf;            // dedup regions (nullable: no score-then-update)
  int32_t dcap;
  int32_t dmax;
  // 1: K1 owns the accounts with 2..K1_SEG_MAX events in the batch (scores all their rows and
  // applies their events); only for a batch in which no account has more, with no update_segments
  // launch behind it. 0: such accounts are scored per row and applied by update_segments.
  int32_t own_short;
  int32_t x_stride;
  int32_t ring_size;
  int32_t n_rows;           // rows covered by the launch (graph bucket)
  int64_t* trace;           // [8 waves][8] phase timestamps (nullable; tools/kbench.py --trace)
  // score-then-update (dbuf != null): the batch's dedup insert ran before K1 (dedup_insert);
  // each quarter-wave applies its request's event when it is the account's only one in the
  // batch; with own_short, an account's first row also applies all of its 2..K1_SEG_MAX events;
  // the other multi-event accounts are applied by update_segments after K1. K1 also clears the
  // region of batch seq + DEDUP_AHEAD.
  UpdateArgs upd;
};


void launch_feature_assemble(const AssembleArgs& a, hipStream_t st);
// standalone event ingestion (event bus / history replay): reset + insert + single + segments
void launch_feature_update(const UpdateArgs& a, hipStream_t st);
// scorer path: dedup insert of the batch (before K1; K1 applies the single-event accounts, and
// with own_short every account of a batch whose accounts have at most K1_SEG_MAX events) ...
void launch_dedup_insert(const UpdateArgs& a, hipStream_t st);
// ... and the tail after K1: per-account apply of the multi-event accounts (not launched by the
// native driver behind an own_short K1)
void launch_update_segments(const UpdateArgs& a, hipStream_t st);

// ---- K2 tree ensemble (complete layout)
struct EnsembleArgs {
  const BatchHdr* hdr;
  const ScoreCfg* cfg;
  const FeatRec* feat;
  const float* X;           // for the heuristic model
  int32_t x_stride;
  const float* ml;          // model output (nullable)
  ResultRec* out;
  ResultRec* host_out;      // nullable: pinned host rows written directly (no D2H copy node)
  unsigned long long* metrics;  // [128] score histogram(101) | actions(4) | ml_high | rows (nullable)
  int32_t n_rows;
  // nullable: host_out is routed - live row i goes to host_out + (p * route_stride bytes) + j rows,
  // route[i] = p * route_c + j (the exchange's compacted rows back into their senders' chunks of
  // the node-shared results region; padding rows are not written)
  const int32_t* route;
  int32_t route_c;
  int32_t route_stride;
};
struct TreeArgs {
  const BatchHdr* hdr;      // nullable: all n_rows live
  const float* X;           // [n][x_stride]
  const float2* nodes;      // [T][2^D-1] (threshold, meta bits)
  const float* leaves;      // [T][2^D][K]
  const float* base;        // [K] (nullable)
  float* out;               // [n][n_out]
  int32_t x_stride;
  int32_t n_rows;
  int32_t n_trees;
  int32_t depth;
  int32_t k;                // targets per leaf
  int32_t n_out;            // output columns (2 in the binary-classifier case)
  int32_t post;             // 0 none, 1 logistic, 2 softmax
  int32_t average;          // 1 = AVERAGE aggregate
  int32_t binary_class;     // -1 unless classifier binary case
  int32_t all_positive;
  int32_t no_finish;        // grouped launch: leave partials for the consumer (mlp_head)
  int32_t all_leq;          // every node BRANCH_LEQ (fast decision path; missing tracks allowed)
  int64_t* trace;           // nullable: phase trace of sample blocks (tools/tree_bench.py)
  int32_t fuse_ens;         // grouped launch: K5 in the finish kernel's epilogue (ml = out)
  EnsembleArgs ens;
  const uint32_t* sets;     // member-set table of the mode-6 nodes (csrc/runtime/trees.h; nullable)
  int32_t n_sets;           // its length in 32-bit words
};
void launch_tree_ensemble(const TreeArgs& a, hipStream_t st);
void launch_tree_ensemble_grouped(const TreeArgs& a, int groups, float* partial, hipStream_t st);

// ---- K2b general trees on the pointer layout (csrc/runtime/trees.h Sparse)
struct TreeSparseArgs {
  const float* X;           // [n][x_stride]
  const int32_t* nodes;     // [N][4] {meta, threshold bits, true child, false child | leaf row}
  const int32_t* roots;     // [T] root node of each tree
  const float* leaf_w;      // [L][K]
  const uint8_t* leaf_has;  // [L][K] target written by the leaf (MIN / MAX)
  const float* base;        // [K] (nullable)
  float* out;               // [n][n_out]
  int32_t x_stride;
  int32_t n_rows;
  int32_t n_trees;
  int32_t depth;            // longest root-to-leaf path (bounds the traversal loop)
  int32_t k;                // targets (<= 64)
  int32_t n_out;
  int32_t post;             // tree_post.h TreePostKind
  int32_t aggregate;        // 0 sum, 1 average, 2 min, 3 max
  int32_t binary_class;     // -1 unless classifier binary case
  int32_t all_positive;
  int32_t feat_w;           // largest feature id + 1 (the staged X tile width)
  const uint32_t* sets;     // member-set table of the mode-6 nodes (csrc/runtime/trees.h; nullable)
  int32_t n_sets;           // its length in 32-bit words
};
void launch_tree_sparse(const TreeSparseArgs& a, int groups, float* partial, hipStream_t st);

// ---- K3 dense layers: Y = act(X W^T + b)
struct GemmArgs {
  const void* X;            // [M][ldx] f32 or bf16
  const void* W;            // bf16 or f32 (w_f32) [N_pad][K_pad] (row n = output column n)
  const float* bias;        // [N] nullable
  void* Y;                  // [M][ldy] f32 or bf16
  const int32_t* m_ptr;     // live rows in device memory (nullable -> M)
  int32_t M, N, K;          // logical sizes; K_pad = round_up(K, 32)
  int32_t ldx, ldy, ldw;
  int32_t x_bf16, y_bf16;
  int32_t act;              // 0 none, 1 relu, 2 sigmoid, 3 tanh
  int32_t w_f32;            // 1: f32 weights, f32 MFMA (v_mfma_f32_16x16x4_f32), reference precision
};
void launch_gemm(const GemmArgs& a, hipStream_t st);
void launch_gemv(const GemmArgs& a, hipStream_t st);  // N == 1 heads

// ---- K3 quantised dense layers (qgemm.hip): int8 x int8 -> int32 on v_mfma_i32_16x16x64_i8,
// Y = act(float(acc + corr[n]) * mult[n] + bias[n]), optionally requantised. A quantised value q
// (uint8 / int8) is stored as the signed byte q - off, off = 128 / 0.
enum QOut : int32_t { QY_F32 = 0, QY_BF16 = 1, QY_Q8 = 2 };
constexpr int Q_MAX_K = 32768;  // acc + corr stays inside int32 up to here
struct QGemmArgs {
  const int8_t* X;          // [M][ldx] stored bytes q_x - off_x
  const int8_t* W;          // [N_pad(128)][ldw = K_pad(64)] w_q - z_w, zero padded
  const int32_t* corr;      // [N] (off_x - z_x) * sum_k W[n][k]
  const float* mult;        // [N] s_x * s_w[n] * alpha
  const float* bias;        // [N] nullable
  void* Y;                  // [M][ldy] f32 / bf16 / stored bytes (y_kind)
  const int32_t* m_ptr;     // live rows in device memory (nullable -> M)
  int32_t M, N, K;
  int32_t ldx, ldy, ldw;
  int32_t y_kind;           // QOut
  int32_t act;              // 0 none, 1 relu, 2 sigmoid, 3 tanh
  float y_scale;            // QY_Q8: Y = clamp(rintf(v / y_scale) + y_zp) - y_off
  int32_t y_zp, y_off;
};
void launch_qgemm(const QGemmArgs& a, hipStream_t st);
int qgemm_tile(int M, int N);  // rows = columns of the output tile launch_qgemm picks (64 | 128)

// QuantizeLinear (F -> Q) / DequantizeLinear (Q -> F) of one [M][N] tensor, per-tensor parameters
struct QuantRowsArgs {
  void* F;                  // [M][ldf] f32 or bf16: read (quantise) or written (dequant)
  int8_t* Q;                // [M][ldq] stored bytes q - off: written (quantise) or read
  const int32_t* m_ptr;     // live rows in device memory (nullable -> M)
  int32_t M, N;
  int32_t ldf, ldq;
  int32_t f_bf16;
  int32_t dequant;          // 0: Q = clamp(rintf(F / scale) + zp) - off; 1: F = (Q + off - zp) * scale
  float scale;
  int32_t zp, off;
};
void launch_quant_rows(const QuantRowsArgs& a, hipStream_t st);

// ---- kernel machines (svm.hip): ai.onnx.ml SVMRegressor / two-class SVMClassifier,
//   dec[m] = sum_i coef[i] * K(x'_m, sv_i) + rho,  x' = x * in_scale + in_shift,  d = x' . sv_i
// on v_mfma_f32_16x16x4_f32, f32 throughout. The epilogue: Platt 1 / (1 + exp(a dec + b)) (flipped
// to 1 - p), else the one-class sign; then v * post_scale + post_shift, then the activation.
enum SvmKernel : int32_t { SVM_LINEAR = 0, SVM_POLY = 1, SVM_RBF = 2, SVM_SIGMOID = 3 };
constexpr int SVM_MAX_F = 256;    // widest input the kernel stages (its X tile lives in LDS)
constexpr int SVM_MAX_DEGREE = 16;
constexpr int SVM_TILE_S = 64;    // support vectors per streamed tile (the table is padded to it)
constexpr int SVM_TILE_K = 32;    // columns per streamed chunk (the table is padded to it)
struct SvmArgs {
  const float* X;           // [M][ldx] f32
  const float* sv;          // [S_pad(64)][f_pad = round_up(F, 32)] zero padded (RBF: centred)
  const float* coef;        // [S_pad]
  const float* sv_norm;     // [S_pad] |sv_i|^2 (RBF; nullable otherwise)
  const float* in_scale;    // [f_pad] input affine (ones / zeros when the model has none)
  const float* in_shift;    // [f_pad]
  float* Y;                 // [M][ldy], column 0
  const int32_t* m_ptr;     // live rows in device memory (nullable -> M)
  int32_t M, F, S;
  int32_t ldx, ldy, f_pad;
  int32_t kernel;           // SvmKernel
  int32_t degree;           // POLY: 0 .. SVM_MAX_DEGREE
  float gamma, coef0, rho;
  int32_t platt;            // 0 none, 1 p = 1 / (1 + exp(a dec + b)), 2 the other class: 1 - p
  float prob_a, prob_b;
  int32_t one_class;        // dec > 0 ? 1 : -1
  float post_scale, post_shift;
  int32_t act;              // 0 none, 2 sigmoid (GemmArgs::act codes)
  int32_t tile;             // rows per workgroup: 0 -> svm_tile(M), else 16 | 32 | 64
};
void launch_svm(const SvmArgs& a, hipStream_t st);
int svm_tile(int M);  // rows per workgroup launch_svm picks (16 | 32 | 64)

// ---- temporal convolutions (conv1d.hip): one layer of a Conv1D / TCN sequence model per launch,
//   out[row][t][o] = act_post(act(b[o] + sum_j sum_c W[o][c][j] x[row][t - pad_left + j dil][c]) + res[row][t][o])
// on v_mfma_f32_16x16x4_f32, f32 throughout; x is zero outside [0, T). Activation buffers are
// channel-last [rows][T][ld] f32, ld a multiple of 4, 16-byte aligned.
constexpr int CONV_MAX_C = 256;      // input / output channels
constexpr int CONV_MAX_K = 8;        // taps
constexpr int CONV_MAX_SPAN = 128;   // dil * (k - 1)
constexpr int CONV_MAX_T = 1024;     // time steps
struct ConvArgs {
  // input: mode 0 dense X f32 [T][x_rows][c_in]; mode 1 per-account event ring (bf16 [C][ev_ring][I],
  // c_in <= I, the seq_src rules of seq_input.h); mode 2 an activation buffer X [rows][T][ldx]
  int32_t mode;
  const float* X;
  int32_t x_rows, ldx;
  const uint16_t* ev;
  const AcctRT* rt;
  const int32_t* slots;     // [rows] (-1 -> all zeros)
  int32_t ev_ring, I;
  const float* W;           // fragment-packed [ceil(c_out / 16)][k][ceil(c_in / 16)][64 lanes][4] (plan.conv_tables)
  const float* bias;        // [round_up(c_out, 16)], zeros past c_out
  const float* res;         // [rows][T][ldr] added after act (nullable)
  float* Y;                 // [rows][T][ldy]; columns [c_out, min(ldy, round_up(c_out, 16))) are written as zeros
  int32_t ldr, ldy;
  const int32_t* m_ptr;     // live rows in device memory (nullable -> n_rows)
  int32_t n_rows, T, c_in, c_out, k, dil, pad_left;
  int32_t act, act_post;    // GemmArgs::act codes
  int32_t tt;               // time steps per workgroup: 0 auto | 32 | 64 (a row's result does not depend on it)
  int32_t per_tap;          // 1: stage each tap's steps on their own (0: when tile + halo fit the LDS)
};
bool conv1d_plan(const ConvArgs& a, int& tt, int& per_tap);   // the tile launch_conv1d picks; false: no tile fits
void launch_conv1d(const ConvArgs& a, hipStream_t st);

enum SeqPoolOp : int32_t { POOL_LAST = 0, POOL_MEAN = 1, POOL_MAX = 2, POOL_SUM = 3 };
struct SeqPoolArgs {
  const float* X;           // [rows][T][ldx]
  void* Y;                  // [rows][ldy] f32 or bf16, columns [0, C)
  const int32_t* m_ptr;
  int32_t n_rows, T, C, ldx, ldy;
  int32_t op;               // SeqPoolOp; max: a NaN in the column gives NaN
  int32_t y_bf16;
};
void launch_seq_pool(const SeqPoolArgs& a, hipStream_t st);

// DAG join of two branches (join.hip): op 0 Y = A + B (na columns), op 1 Y = [A | B]
struct JoinArgs {
  const void* A;
  const void* B;
  void* Y;
  const int32_t* m_ptr;     // live rows in device memory (nullable -> M)
  int32_t M, na, nb, op;
  int32_t lda, ldb, ldy;
  int32_t a_bf16, b_bf16, y_bf16;
};
void launch_join(const JoinArgs& a, hipStream_t st);

// Row ops on one [M][N] activation tensor (rowops.hip): layernorm and softmax over each row,
// and the elementwise activations the dense / head epilogues do not carry
enum RowOp : int32_t { ROW_LAYERNORM = 0, ROW_SOFTMAX = 1, ROW_ACT = 2 };
// act codes 0-3 are the dense epilogue's (GemmArgs::act)
enum RowAct : int32_t { RA_NONE = 0, RA_RELU = 1, RA_SIGMOID = 2, RA_TANH = 3, RA_LEAKY_RELU = 4, RA_ELU = 5,
                        RA_SELU = 6, RA_SOFTPLUS = 7, RA_HARD_SIGMOID = 8, RA_GELU = 9, RA_GELU_TANH = 10,
                        RA_CLIP = 11, RA_PRELU = 12 };
struct RowArgs {
  const void* X;            // [M][ldx] f32 or bf16
  void* Y;                  // [M][ldy] f32 or bf16
  const float* gamma;       // [N]: layernorm scale (required); prelu per-column slope (nullable -> p0)
  const float* beta;        // [N]: layernorm bias (nullable)
  const int32_t* m_ptr;     // live rows in device memory (nullable -> M)
  int32_t M, N;
  int32_t ldx, ldy;
  int32_t x_bf16, y_bf16;
  int32_t op;               // RowOp
  int32_t act;              // RowAct (op ROW_ACT)
  float p0, p1;             // act parameters: alpha | alpha, gamma (selu) | alpha, beta (hard_sigmoid) | lo, hi (clip)
  float eps;                // layernorm
};
void launch_row(const RowArgs& a, hipStream_t st);

// Column assembly (columns.hip, models/plan.py ColumnStep): Y[:M, :out_width] = a per-column program
// of X[:M, :in_width]. One ColRecord per output column, evaluated in this order: x = X[r][src];
// impute (x = hit ? value : x; hit = isnan(x) with COL_IMP_NAN, else x == replaced); the affine
// (x - sub) * mul, an f32 subtract then an f32 multiply; the mode.
enum ColMode : int32_t { COL_PASS = 0, COL_ONEHOT = 1, COL_BINARIZE = 2, COL_ZERO = 3 };  // flags & COL_MODE_MASK
constexpr int32_t COL_MODE_MASK = 0xf, COL_IMPUTE = 0x10, COL_IMP_NAN = 0x20, COL_AFFINE = 0x40;
constexpr int COL_MAX_IN = 256;     // widest input: the X tile lives in LDS
constexpr int COL_MAX_OUT = 4096;
constexpr int COL_TILE_ROWS = 32;   // rows per workgroup
struct ColRecord {          // 32 bytes: two 16-byte loads
  int32_t src;              // input column, < in_width
  int32_t flags;            // ColMode | COL_IMPUTE | COL_IMP_NAN | COL_AFFINE
  float replaced, value;    // impute
  float sub, mul;           // affine
  float arg;                // COL_ONEHOT: the category (truncf(x) == arg); COL_BINARIZE: the threshold (x > arg)
  float pad;
};
struct ColArgs {
  const float* X;           // [M][ldx] f32
  void* Y;                  // [M][ldy] f32 or bf16
  const ColRecord* tab;     // [round_up(out_width, 4)]; the padding records are COL_ZERO on column 0
  const int32_t* m_ptr;     // live rows in device memory (nullable -> M)
  int32_t M, in_width, out_width;
  int32_t ldx, ldy;
  int32_t y_bf16;
};
void launch_col_assemble(const ColArgs& a, hipStream_t st);

// dense(N1) + act1 + dense(N1 -> 1) + act2 fused; W1 bf16 [N1_pad(64)][k_pad(32)]
// ---- K5 ensemble + action + metrics
struct HeadArgs {
  const void* X;
  const void* W1;           // bf16, or f32 when w1_f32 (reference-precision head)
  const float* b1;          // [N1] nullable
  const float* w2;          // [N1] f32
  float b2;
  float* Y;                 // [M][ldy] f32 (column 0)
  const int32_t* m_ptr;
  int32_t M, K, N1, k_pad;
  int32_t ldx, ldy;
  int32_t x_bf16;
  int32_t act1, act2;
  // optional: X is a tree partial slab [groups][M][K] to be reduced (+base, /T) while staging
  const float* partial;
  const float* pbase;
  int32_t groups;
  int32_t p_average;
  int32_t p_ntrees;
  int64_t* trace;           // nullable: phase trace of 8 sample blocks (tools/kbench.py)
  // optional fused K5: each block runs the ensemble of its rows on the Y values it computed
  // (ml = Y[row], the plan's ml_col 0); the standalone ensemble launch is then skipped
  int32_t fuse_ens;
  EnsembleArgs ens;
  int32_t w1_f32;           // 1: f32 W1 / activations, v_mfma_f32_16x16x4_f32 (no bf16 rounding anywhere)
};
void launch_mlp_head(const HeadArgs& a, hipStream_t st);

// cfg3 stacked model in one launch (trees.hip tree_head_kernel): grouped K = 32 tree ensemble
// whose last-arriving group block per 64-row tile runs the f32 head (+ fused K5) on the tile.
// h.partial / h.groups describe the slab the tree blocks write; tile_cnt: zeroed uint32 per tile.
bool tree_head_supported(const TreeArgs& a, const HeadArgs& h, int groups);
void launch_tree_head(const TreeArgs& a, const HeadArgs& h, int groups, float* partial, unsigned int* tile_cnt,
                      hipStream_t st);

void launch_ensemble(const EnsembleArgs& a, hipStream_t st);

// Cluster counters of the weight-stationary GRU kernels (gru_ws.hip, gru_wsx.hip): a member
// whose bounded wait times out stores this value into its cluster's counters before it exits.
// Every later wait on them then fails as well (no launch can add its way back to a target from
// here), so counters that a failed launch left part-advanced are never passed early; the host
// zeroes them when it falls back (GruPack.disable_ws) - a successful launch leaves them at 0.
constexpr int32_t kClusterPoison = -(1 << 30);

// ---- K4 GRU (1-2 stacked ONNX GRU layers, forward, layout 0) + optional N=1 head
// Weights are fragment-packed on the host: P[nt][ks][lane][8] = W[nt*16 + (lane&15)]
// [ks*32 + 8*(lane>>4) + j], so one wave load of a B fragment is 1 KiB contiguous.
struct GruLayerArgs {
  const uint16_t* W;        // packed bf16, N = 3H rows, K = kx_pad (input dim padded to 32)
  const uint16_t* R;        // packed bf16, N = 3H rows, K = H
  const float* bias;        // [6H]: Wb z,r,h | Rb z,r,h
  int32_t kx_pad;
  int32_t lbr;              // linear_before_reset
  const uint16_t* W_lo;     // split mode: bf16 residuals (w - bf16(w)), same fragment order
  const uint16_t* R_lo;
};
struct GruArgs {
  GruLayerArgs layer[2];
  int32_t n_layers, H, T, I;
  // input: mode 0 dense X f32 [T][x_rows][I]; mode 1 per-account event ring (bf16 [C][ring][I])
  int32_t mode;
  const float* X;
  int32_t x_rows;
  const uint16_t* ev;
  const AcctRT* rt;
  const int32_t* slots;     // [rows] (-1 -> empty history)
  int32_t ev_ring;
  const int32_t* m_ptr;     // live row count on device (nullable)
  int32_t n_rows;
  float* yh;                // [rows][H] last layer's final hidden state (nullable)
  const float* head_w;      // [H] (nullable): out[r] = act(h . w + b)
  float head_b;
  int32_t head_act;         // 0 none, 2 sigmoid
  float* out;               // [rows]
  int32_t tile_rows;        // 0 auto | 16 | 32 rows per workgroup
  int32_t waves;            // 0 auto (4) | 8 waves per workgroup (H >= 128)
  int32_t pipeline;         // 2 layers: layer-pipelined kernel (layer 1 @ t || layer 2 @ t-1)
  // weight-stationary cluster path (gru_ws.hip), used when the workspace is given and the
  // model is the 2 x 256, linear_before_reset = 1, input <= 32 shape
  int32_t ws;               // 0 off | 1 use when eligible | 2 two-half pipeline | 3 two 64-row clusters per CU
  // the workspace is sized in the kernel's clusters: 128 rows (ws = 1, 2), 64 rows (ws = 3: two per
  // 128-row cluster of capacity) or 32 rows (split mode, gru_wsx.hip, below)
  int32_t ws_clusters;      // workspace capacity in 128-row clusters (split mode: 32-row clusters)
  int32_t* ws_sync;         // [2 ws_clusters][16] step counters (back to 0 after every launch)
  uint16_t* ws_x;           // [ws_clusters][2][8][2][128][32] bf16 hand-off slabs (ws = 3: [2 ws_clusters][2][8][2][64][32])
  float* ws_part;           // [ws_clusters][8][128] head partials (ws = 3: [2 ws_clusters][8][64])
  int32_t* ws_err;          // [1] set when a cluster was not co-resident (bounded wait expired)
  int64_t* ws_trace;        // 64 * 8 + 4 + 1024 words (nullable): per-step phase timestamps of workgroup 0, clocks,
                            // workgroup placement (tools/gru_ws_trace.py, tools/gru_wsx_trace.py)
  int32_t split;            // 1: f32-faithful bf16 hi/lo pairs, three MFMAs per product (gru.hip x3)
  int32_t reverse;          // 1: ONNX direction=reverse (every layer): time steps read last to first
  // ONNX sequence_lens: a row is updated on its live steps only and holds h on every other one.
  // Live window of actual time indices: mode 0 [0, lens[row]), mode 1 [T - min(ev_count, T), T).
  // Batch-parallel kernels only (never the weight-stationary clusters); T <= 65535.
  int32_t masked;
  const int32_t* lens;      // [rows], mode 0 only (nullable -> every row full length)
};
void launch_gru(const GruArgs& a, hipStream_t st);
void launch_gru_masked(const GruArgs& a, hipStream_t st);  // gru_masked.hip; launch_gru routes a.masked here
bool gru_ws_eligible(const GruArgs& a);
void launch_gru_ws(const GruArgs& a, hipStream_t st);
int gru_ws_clusters(int n_rows);
int gru_ws2_clusters(int n_rows);  // 64-row clusters (ws = 3)
// split (f32-faithful) weight-stationary clusters of 16 workgroups x 32 rows (gru_wsx.hip);
// the workspace is then sized in 32-row clusters: ws_sync [clusters][16], ws_x
// [clusters][2][16][4][32][16] bf16, ws_part [clusters][16][32]
bool gru_wsx_eligible(const GruArgs& a);
void launch_gru_wsx(const GruArgs& a, hipStream_t st);
int gru_wsx_clusters(int n_rows);

// ---- K4 LSTM (1-2 stacked ONNX LSTM layers, gates i, o, f, c, zero initial states) + optional
// N=1 head: the batch-parallel design of the GRU kernel (lstm.hip). Weights fragment-packed as
// above with N = 4H rows (gate-major: the gate g tile of hidden tile ht is column tile g*H/16 + ht).
struct LstmLayerArgs {
  const uint16_t* W;        // packed bf16, N = 4H rows, K = kx_pad
  const uint16_t* R;        // packed bf16, N = 4H rows, K = H
  const float* bias;        // [8H]: Wb i,o,f,c | Rb i,o,f,c
  int32_t kx_pad;
  const uint16_t* W_lo;     // split mode: bf16 residuals, same fragment order
  const uint16_t* R_lo;
};
struct LstmArgs {
  LstmLayerArgs layer[2];
  int32_t n_layers, H, T, I;
  int32_t mode;             // 0 dense X f32 [T][x_rows][I]; 1 per-account event ring (bf16 [C][ring][I])
  const float* X;
  int32_t x_rows;
  const uint16_t* ev;
  const AcctRT* rt;
  const int32_t* slots;     // [rows] (-1 -> empty history)
  int32_t ev_ring;
  const int32_t* m_ptr;     // live row count on device (nullable)
  int32_t n_rows;
  float* yh;                // [rows][H] last layer's final hidden state (nullable)
  const float* head_w;      // [H] (nullable): out[r] = act(h . w + b)
  float head_b;
  int32_t head_act;         // 0 none, 2 sigmoid
  float* out;               // [rows]
  int32_t tile_rows;        // 0 / 16 | 32 rows per workgroup (32 only where the LDS allows)
  int32_t split;            // 1: f32-faithful bf16 hi/lo pairs, three MFMAs per product
  int32_t reverse;          // 1: ONNX direction=reverse: time steps read last to first
  int32_t masked;           // ONNX sequence_lens, as GruArgs.masked (h and c are held)
  const int32_t* lens;      // [rows], mode 0 only (nullable -> every row full length)
};
void launch_lstm(const LstmArgs& a, hipStream_t st);
void launch_lstm_masked(const LstmArgs& a, hipStream_t st);  // lstm_masked.hip; launch_lstm routes a.masked here
// rows per workgroup launch_lstm uses (16, or 32 when requested and the activation tiles fit the LDS)
int lstm_tile_rows(int H, int kx_pad, int split, int requested);

// ---- K9 LTV / churn / segment
struct LtvArgs {
  const float* pf;          // [B][25] player features (golden.ltv.PLAYER_COLUMNS), or the table when slots != null
  const int32_t* slots;     // [B] rows of the device-resident player table (nullable; -1 -> empty profile)
  const float* ltv_model;   // [B] learned LTV (nullable -> formula)
  float* out;               // [B][6]: ltv, churn, survival, confidence, segment, nba
  int32_t B;
};
void launch_ltv(const LtvArgs& a, hipStream_t st);

// LTV model input from the device-resident tables: X[r] = [sign*log1p|pf[slot]| (25) | ext[slot] (ext_w)]
struct LtvAssembleArgs {
  const int32_t* slots;
  const float* pf_tab;      // [C][25]
  const float* ext_tab;     // [C][ext_w] (nullable)
  int32_t ext_w;
  float* X;                 // [rows][x_w], x_w = 25 + ext_w
  int32_t x_w;
  const int32_t* m_ptr;     // live rows (nullable)
  int32_t n_rows;
};
void launch_ltv_assemble(const LtvAssembleArgs& a, hipStream_t st);

// ---- K3 fused MLP chain (mlp_fused.hip): up to 8 dense layers with the activation tile in LDS,
// the last one followed by an N -> 1 head; optional LTV input gather and K9 epilogue
constexpr int MC_MAX_LAYERS = 8;
struct MlpChainArgs {
  const float* X;           // dense input [rows][ldx] f32 (when slots == null)
  int32_t ldx;
  const int32_t* slots;     // LTV gather: player slots [rows] (-1: empty profile)
  const float* pf_tab;      // [C][25]
  const float* ext_tab;     // [C][ext_w] (nullable)
  int32_t ext_w;
  int32_t in_w;             // staged input width = K[0] (multiple of 64)
  int32_t in_live;          // real input columns (<= in_w; the rest are zero)
  const int32_t* m_ptr;     // live rows in device memory (nullable)
  int32_t n_rows;
  int32_t n_layers;
  const uint16_t* W[MC_MAX_LAYERS];  // bf16 [N][K] row-major
  const float* bias[MC_MAX_LAYERS];  // [N] (nullable)
  int32_t N[MC_MAX_LAYERS];          // multiple of 64, <= 512
  int32_t K[MC_MAX_LAYERS];          // multiple of 64, <= 512; K[l] == N[l-1]
  int32_t act[MC_MAX_LAYERS];
  const float* w2;          // head [N_last] f32
  float b2;
  int32_t act2;
  float* ml;                // [rows] head output (nullable)
  float* ltv_out;           // [rows][6] K9 output (nullable; needs slots + pf_tab)
  int32_t rows_per_block;   // 16, 32 (default) or 64 rows per workgroup
  int32_t waves;            // 4 (default) or 8 (32 rows; each wave owns N/8 columns)
  const uint16_t* W_lo[MC_MAX_LAYERS];  // split (f32-faithful) mode: bf16 residuals w - bf16(w)
  int32_t split;            // 1: three-MFMA bf16 pairs (hi*hi + hi*lo + lo*hi)
};
void launch_mlp_chain(const MlpChainArgs& a, hipStream_t st);

}  // namespace igp
