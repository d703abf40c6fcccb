// CPU reference executor: float32 tensors, double accumulation for matrix products.
#include "executor.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <numeric>
#include <set>
#include <stdexcept>

#include "columns.h"
#include "conv.h"

namespace igp::exec {
namespace {

using onnx::FLOAT;
using onnx::INT64;

Tensor make(const std::vector<int64_t>& dims, int32_t dtype = FLOAT) {
  Tensor t;
  t.dims = dims;
  t.dtype = dtype;
  if (dtype == FLOAT) t.f.assign(t.numel(), 0.f);
  else t.i.assign(t.numel(), 0);
  return t;
}

std::vector<float> as_float(const Tensor& t) {
  if (t.dtype == FLOAT) return t.f;
  return std::vector<float>(t.i.begin(), t.i.end());
}

std::vector<int64_t> as_int(const Tensor& t) {
  if (t.dtype == INT64 || t.dtype == onnx::INT32) return t.i;
  std::vector<int64_t> r;
  for (float v : t.f) r.push_back(cols::float_to_int64(v));  // NaN / out of range: INT64_MIN, defined
  return r;
}

int64_t norm_axis(int64_t a, size_t rank) {
  if (a < 0) a += int64_t(rank);
  if (a < 0 || a >= int64_t(rank) + 1) throw std::runtime_error("axis out of range");
  return a;
}

// numpy-style broadcasting elementwise binary op on float tensors
Tensor binary(const Tensor& A, const Tensor& B, const std::function<float(float, float)>& op) {
  const auto a = as_float(A), b = as_float(B);
  size_t r = std::max(A.dims.size(), B.dims.size());
  std::vector<int64_t> da(r, 1), db(r, 1), dout(r);
  std::copy(A.dims.begin(), A.dims.end(), da.begin() + (r - A.dims.size()));
  std::copy(B.dims.begin(), B.dims.end(), db.begin() + (r - B.dims.size()));
  for (size_t k = 0; k < r; ++k) {
    if (da[k] != db[k] && da[k] != 1 && db[k] != 1) throw std::runtime_error("broadcast: incompatible shapes");
    dout[k] = std::max(da[k], db[k]);
  }
  Tensor out = make(dout);
  std::vector<int64_t> sa(r), sb(r);
  int64_t ma = 1, mb = 1;
  for (int k = int(r) - 1; k >= 0; --k) {
    sa[k] = da[k] == 1 ? 0 : ma; ma *= da[k];
    sb[k] = db[k] == 1 ? 0 : mb; mb *= db[k];
  }
  std::vector<int64_t> idx(r, 0);
  const int64_t n = out.numel();
  for (int64_t e = 0; e < n; ++e) {
    int64_t oa = 0, ob = 0;
    for (size_t k = 0; k < r; ++k) { oa += idx[k] * sa[k]; ob += idx[k] * sb[k]; }
    out.f[e] = op(a[oa], b[ob]);
    for (int k = int(r) - 1; k >= 0; --k) {
      if (++idx[k] < dout[k]) break;
      idx[k] = 0;
    }
  }
  return out;
}

Tensor unary(const Tensor& A, const std::function<float(float)>& op) {
  Tensor out = make(A.dims);
  auto a = as_float(A);
  for (size_t k = 0; k < a.size(); ++k) out.f[k] = op(a[k]);
  return out;
}

inline float sigmoid(float x) { return 1.f / (1.f + std::exp(-x)); }

// ---- ai.onnx QDQ quantisation (opset 10 / 13 forms). Tensors stay float: a quantised value is an
// integer of at most 9 bits held in a float, tagged with its type in Tensor::elem.
const char* const kQdqOnly = " is not supported: quantised models run in the QDQ format (QuantizeLinear / "
                             "DequantizeLinear around float Gemm / MatMul)";

void qdq_attrs(const onnx::Node& n) {
  if (n.geti("block_size", 0) != 0) throw std::runtime_error(n.op_type + ": block_size (blocked quantisation) is not supported");
  if (n.geti("saturate", 1) != 1) throw std::runtime_error(n.op_type + ": saturate=0 is not supported");
  if (const auto* a = n.attr("output_dtype"))
    if (a->i != 0 && a->i != onnx::UINT8 && a->i != onnx::INT8)
      throw std::runtime_error(n.op_type + ": output_dtype " + std::to_string(a->i) + " is not supported (uint8 and int8 only)");
}

// the quantised type a zero point gives (absent: uint8); its range in lo / hi
int32_t quant_type(const std::string& op, const Tensor* zp, int32_t dflt, float& lo, float& hi) {
  const int32_t t = zp ? zp->elem : dflt;
  if (t == onnx::UINT8) { lo = 0.f; hi = 255.f; }
  else if (t == onnx::INT8) { lo = -128.f; hi = 127.f; }
  else throw std::runtime_error(op + ": zero point of ONNX type " + std::to_string(t) + " is not supported (uint8 and int8 only)");
  return t;
}

Tensor quantize_linear(const onnx::Node& n, const Tensor& x, const Tensor& scale, const Tensor* zp) {
  qdq_attrs(n);
  if (x.dtype != FLOAT) throw std::runtime_error("QuantizeLinear: the input must be a float tensor");
  if (scale.dtype != FLOAT || scale.numel() != 1 || (zp && zp->numel() != 1))
    throw std::runtime_error("QuantizeLinear: per-axis quantisation of activations is not supported (one scale, one zero point)");
  float lo, hi;
  const int32_t a_out = int32_t(n.geti("output_dtype", 0));
  const int32_t t = quant_type("QuantizeLinear", zp, a_out ? a_out : int32_t(onnx::UINT8), lo, hi);
  const float s = scale.f[0], z = zp ? float(zp->i[0]) : 0.f;
  Tensor y = make(x.dims);
  y.elem = t;
  // saturate(round_half_even(x / s) + z): a true float division, rint in the default rounding mode
  for (size_t k = 0; k < x.f.size(); ++k) y.f[k] = std::min(hi, std::max(lo, std::rint(x.f[k] / s) + z));
  return y;
}

Tensor dequantize_linear(const onnx::Node& n, const Tensor& x, const Tensor& scale, const Tensor* zp) {
  qdq_attrs(n);
  if (scale.dtype != FLOAT) throw std::runtime_error("DequantizeLinear: the scale must be a float tensor");
  const bool is_int = x.dtype != FLOAT;  // an initializer: uint8 / int8 weights, int32 bias
  if (is_int && x.elem != onnx::UINT8 && x.elem != onnx::INT8 && x.elem != onnx::INT32)
    throw std::runtime_error("DequantizeLinear: input of ONNX type " + std::to_string(x.elem) + " is not supported (uint8, int8, int32)");
  if (zp && zp->dtype == FLOAT) throw std::runtime_error("DequantizeLinear: the zero point must be an integer tensor");
  if (zp && zp->numel() != scale.numel()) throw std::runtime_error("DequantizeLinear: scale and zero point differ in size");
  const int64_t ns = scale.numel();
  int64_t len = 1, inner = 1;
  if (ns != 1) {  // per-axis: weights and biases only
    if (!is_int) throw std::runtime_error("DequantizeLinear: per-axis quantisation of activations is not supported");
    const int64_t ax = norm_axis(n.geti("axis", 1), x.dims.size());
    if (ax >= int64_t(x.dims.size()) || x.dims[ax] != ns)
      throw std::runtime_error("DequantizeLinear: the scale length differs from the axis dimension");
    len = ns;
    for (size_t d = ax + 1; d < x.dims.size(); ++d) inner *= x.dims[d];
  }
  Tensor y = make(x.dims);
  const int64_t total = x.numel();
  for (int64_t e = 0; e < total; ++e) {
    const int64_t c = len == 1 ? 0 : (e / inner) % len;
    const double q = is_int ? double(x.i[e]) : double(x.f[e]);
    const double z = zp ? double(zp->i[c]) : 0.0;
    y.f[e] = float((q - z) * double(scale.f[c]));  // exact integer difference, one rounding
  }
  return y;
}

Tensor gemm(const onnx::Node& n, const Tensor& A, const Tensor& B, const Tensor* C) {
  const float alpha = n.getf("alpha", 1.f), beta = n.getf("beta", 1.f);
  const bool ta = n.geti("transA", 0), tb = n.geti("transB", 0);
  if (A.dims.size() != 2 || B.dims.size() != 2) throw std::runtime_error("Gemm: 2-D inputs required");
  const int64_t M = ta ? A.dims[1] : A.dims[0], K = ta ? A.dims[0] : A.dims[1];
  const int64_t K2 = tb ? B.dims[1] : B.dims[0], N = tb ? B.dims[0] : B.dims[1];
  if (K != K2) throw std::runtime_error("Gemm: inner dimensions differ");
  Tensor Y = make({M, N});
  const auto& a = A.f;
  const auto& b = B.f;
  for (int64_t i = 0; i < M; ++i)
    for (int64_t j = 0; j < N; ++j) {
      double s = 0;
      for (int64_t k = 0; k < K; ++k) {
        float av = ta ? a[k * M + i] : a[i * K + k];
        float bv = tb ? b[j * K + k] : b[k * N + j];
        s += double(av) * double(bv);
      }
      Y.f[i * N + j] = float(alpha * s);
    }
  if (C && beta != 0.f) {
    Tensor c = *C;
    Y = binary(Y, c, [beta](float y, float cv) { return y + beta * cv; });
  }
  return Y;
}

Tensor matmul(const Tensor& A, const Tensor& B) {
  if (B.dims.size() != 2 || A.dims.size() < 1) throw std::runtime_error("MatMul: B must be 2-D");
  const int64_t K = A.dims.back(), N = B.dims[1];
  if (B.dims[0] != K) throw std::runtime_error("MatMul: inner dimensions differ");
  const int64_t M = A.numel() / K;
  std::vector<int64_t> od = A.dims;
  od.back() = N;
  Tensor Y = make(od);
  for (int64_t i = 0; i < M; ++i)
    for (int64_t j = 0; j < N; ++j) {
      double s = 0;
      for (int64_t k = 0; k < K; ++k) s += double(A.f[i * K + k]) * double(B.f[k * N + j]);
      Y.f[i * N + j] = float(s);
    }
  return Y;
}

// The lengths of a GRU / LSTM node's optional sequence_lens input [B] (int32, each in [0, S]); S
// for every row without one.
std::vector<int64_t> seq_lens(const char* op, const Tensor* lens, int64_t Bn, int64_t S) {
  std::vector<int64_t> len(Bn, S);
  if (!lens) return len;
  const std::string o(op);
  if (lens->dtype != onnx::INT32) throw std::runtime_error(o + ": sequence_lens must be an int32 tensor");
  if (lens->dims.size() != 1 || lens->dims[0] != Bn || int64_t(lens->i.size()) != Bn)
    throw std::runtime_error(o + ": sequence_lens must hold one length per batch row");
  for (int64_t b = 0; b < Bn; ++b) {
    if (lens->i[b] < 0 || lens->i[b] > S)
      throw std::runtime_error(o + ": sequence_lens value " + std::to_string(lens->i[b]) + " is outside [0, " +
                               std::to_string(S) + "]");
    len[b] = lens->i[b];
  }
  return len;
}

// ONNX GRU (gates z, r, h), activations sigmoid/tanh, directions forward / reverse /
// bidirectional. layout 0: X [S][B][I], Y [S][D][B][H], Y_h / initial_h [D][B][H];
// layout 1 (batch-major): X [B][S][I], Y [B][S][D][H], Y_h / initial_h [B][D][H].
// sequence_lens: row b is updated on the steps whose time index t < lens[b] and holds its state on
// the others (reverse starts at t = lens[b] - 1); Y stays zero there, Y_h is the held state.
void gru(const onnx::Node& n, const Tensor& X, const Tensor& W, const Tensor& R, const Tensor* Bp,
         const Tensor* lens, const Tensor* h0, Tensor& Y, Tensor& Yh) {
  const int64_t H = n.geti("hidden_size", R.dims.back());
  const bool lbr = n.geti("linear_before_reset", 0);
  const int64_t layout = n.geti("layout", 0);
  if (layout != 0 && layout != 1) throw std::runtime_error("GRU: layout must be 0 or 1");
  std::string dir = n.gets("direction", "forward");
  if (dir != "forward" && dir != "reverse" && dir != "bidirectional") throw std::runtime_error("GRU: direction");
  const int64_t D = dir == "bidirectional" ? 2 : 1;
  if (X.dims.size() != 3) throw std::runtime_error("GRU: X must be rank 3");
  const int64_t S = layout ? X.dims[1] : X.dims[0], Bn = layout ? X.dims[0] : X.dims[1], I = X.dims[2];
  if (W.dims[0] != D || W.dims[1] != 3 * H || W.dims[2] != I) throw std::runtime_error("GRU: W shape");
  if (R.dims[0] != D || R.dims[1] != 3 * H || R.dims[2] != H) throw std::runtime_error("GRU: R shape");
  Y = layout ? make({Bn, S, D, H}) : make({S, D, Bn, H});
  Yh = layout ? make({Bn, D, H}) : make({D, Bn, H});
  // element offsets of (t, b) in X, (t, d, b) in Y and (d, b) in Y_h / initial_h
  auto xo = [&](int64_t t, int64_t b) { return (layout ? b * S + t : t * Bn + b) * I; };
  auto yo = [&](int64_t t, int64_t d, int64_t b) { return (layout ? (b * S + t) * D + d : (t * D + d) * Bn + b) * H; };
  auto ho = [&](int64_t d, int64_t b) { return (layout ? b * D + d : d * Bn + b) * H; };
  std::vector<double> hz(H), hr(H), hh(H), xz(H), xr(H), xh(H);
  const std::vector<int64_t> len = seq_lens("GRU", lens, Bn, S);
  for (int64_t d = 0; d < D; ++d) {
    const bool rev = dir == "reverse" || (D == 2 && d == 1);
    const float* w = &W.f[d * 3 * H * I];
    const float* r = &R.f[d * 3 * H * H];
    std::vector<float> bias(6 * H, 0.f);
    if (Bp) std::copy(Bp->f.begin() + d * 6 * H, Bp->f.begin() + (d + 1) * 6 * H, bias.begin());
    for (int64_t b = 0; b < Bn; ++b) {
      std::vector<float> h(H, 0.f);
      if (h0) std::copy(h0->f.begin() + ho(d, b), h0->f.begin() + ho(d, b) + H, h.begin());
      for (int64_t st = 0; st < S; ++st) {
        const int64_t t = rev ? S - 1 - st : st;
        if (t >= len[b]) continue;
        const float* x = &X.f[xo(t, b)];
        for (int64_t j = 0; j < H; ++j) {
          double az = 0, ar = 0, ah = 0, bz = 0, br = 0, bh = 0;
          for (int64_t k = 0; k < I; ++k) {
            az += double(w[j * I + k]) * x[k];
            ar += double(w[(H + j) * I + k]) * x[k];
            ah += double(w[(2 * H + j) * I + k]) * x[k];
          }
          for (int64_t k = 0; k < H; ++k) {
            bz += double(r[j * H + k]) * h[k];
            br += double(r[(H + j) * H + k]) * h[k];
          }
          xz[j] = az; xr[j] = ar; xh[j] = ah; hz[j] = bz; hr[j] = br;
          (void)bh;
        }
        std::vector<float> rg(H), zg(H);
        for (int64_t j = 0; j < H; ++j) {
          zg[j] = sigmoid(float(xz[j] + hz[j] + bias[j] + bias[3 * H + j]));
          rg[j] = sigmoid(float(xr[j] + hr[j] + bias[H + j] + bias[4 * H + j]));
        }
        for (int64_t j = 0; j < H; ++j) {
          double acc = 0;
          if (lbr) {
            for (int64_t k = 0; k < H; ++k) acc += double(r[(2 * H + j) * H + k]) * h[k];
            hh[j] = rg[j] * (acc + bias[5 * H + j]);
          } else {
            for (int64_t k = 0; k < H; ++k) acc += double(r[(2 * H + j) * H + k]) * (rg[k] * h[k]);
            hh[j] = acc + bias[5 * H + j];
          }
        }
        for (int64_t j = 0; j < H; ++j) {
          float nt = std::tanh(float(xh[j] + bias[2 * H + j] + hh[j]));
          h[j] = (1.f - zg[j]) * nt + zg[j] * h[j];
        }
        std::copy(h.begin(), h.end(), Y.f.begin() + yo(t, d, b));
      }
      std::copy(h.begin(), h.end(), Yh.f.begin() + ho(d, b));
    }
  }
}

// ONNX LSTM (gates i, o, f, c), default activations sigmoid / tanh / tanh, optional peepholes
// P [D][3H] (i, o, f), directions and layouts as for the GRU above; Y_c / initial_c are shaped
// like Y_h / initial_h. Products accumulate in double, the gates are float, as in gru().
void lstm(const onnx::Node& n, const Tensor& X, const Tensor& W, const Tensor& R, const Tensor* Bp,
          const Tensor* lens, const Tensor* h0, const Tensor* c0, const Tensor* Pp, Tensor& Y, Tensor& Yh,
          Tensor& Yc) {
  const int64_t H = n.geti("hidden_size", R.dims.back());
  const int64_t layout = n.geti("layout", 0);
  if (layout != 0 && layout != 1) throw std::runtime_error("LSTM: layout must be 0 or 1");
  std::string dir = n.gets("direction", "forward");
  if (dir != "forward" && dir != "reverse" && dir != "bidirectional") throw std::runtime_error("LSTM: direction");
  const int64_t D = dir == "bidirectional" ? 2 : 1;
  if (auto a = n.attr("activations")) {
    static const char* const def[3] = {"Sigmoid", "Tanh", "Tanh"};
    if (int64_t(a->strings.size()) != 3 * D) throw std::runtime_error("LSTM: activations must name 3 functions per direction");
    for (size_t k = 0; k < a->strings.size(); ++k)
      if (a->strings[k] != def[k % 3])
        throw std::runtime_error("LSTM: activations other than Sigmoid / Tanh / Tanh are not supported (" + a->strings[k] + ")");
  }
  if (n.attr("activation_alpha") || n.attr("activation_beta"))
    throw std::runtime_error("LSTM: activation_alpha / activation_beta are not supported");
  if (n.attr("clip")) throw std::runtime_error("LSTM: clip is not supported");
  if (n.geti("input_forget", 0) != 0) throw std::runtime_error("LSTM: input_forget = 1 is not supported");
  if (X.dims.size() != 3) throw std::runtime_error("LSTM: X must be rank 3");
  const int64_t S = layout ? X.dims[1] : X.dims[0], Bn = layout ? X.dims[0] : X.dims[1], I = X.dims[2];
  if (W.dims.size() != 3 || W.dims[0] != D || W.dims[1] != 4 * H || W.dims[2] != I) throw std::runtime_error("LSTM: W shape");
  if (R.dims.size() != 3 || R.dims[0] != D || R.dims[1] != 4 * H || R.dims[2] != H) throw std::runtime_error("LSTM: R shape");
  if (Bp && Bp->numel() != D * 8 * H) throw std::runtime_error("LSTM: B shape");
  if (Pp && Pp->numel() != D * 3 * H) throw std::runtime_error("LSTM: P shape");
  if (h0 && h0->numel() != D * Bn * H) throw std::runtime_error("LSTM: initial_h shape");
  if (c0 && c0->numel() != D * Bn * H) throw std::runtime_error("LSTM: initial_c shape");
  Y = layout ? make({Bn, S, D, H}) : make({S, D, Bn, H});
  Yh = layout ? make({Bn, D, H}) : make({D, Bn, H});
  Yc = Yh;
  auto xo = [&](int64_t t, int64_t b) { return (layout ? b * S + t : t * Bn + b) * I; };
  auto yo = [&](int64_t t, int64_t d, int64_t b) { return (layout ? (b * S + t) * D + d : (t * D + d) * Bn + b) * H; };
  auto ho = [&](int64_t d, int64_t b) { return (layout ? b * D + d : d * Bn + b) * H; };
  std::vector<double> g(4 * H);
  const std::vector<int64_t> len = seq_lens("LSTM", lens, Bn, S);
  for (int64_t d = 0; d < D; ++d) {
    const bool rev = dir == "reverse" || (D == 2 && d == 1);
    const float* w = &W.f[d * 4 * H * I];
    const float* r = &R.f[d * 4 * H * H];
    std::vector<float> bias(8 * H, 0.f), peep(3 * H, 0.f);
    if (Bp) std::copy(Bp->f.begin() + d * 8 * H, Bp->f.begin() + (d + 1) * 8 * H, bias.begin());
    if (Pp) std::copy(Pp->f.begin() + d * 3 * H, Pp->f.begin() + (d + 1) * 3 * H, peep.begin());
    for (int64_t b = 0; b < Bn; ++b) {
      std::vector<float> h(H, 0.f), c(H, 0.f);
      if (h0) std::copy(h0->f.begin() + ho(d, b), h0->f.begin() + ho(d, b) + H, h.begin());
      if (c0) std::copy(c0->f.begin() + ho(d, b), c0->f.begin() + ho(d, b) + H, c.begin());
      for (int64_t st = 0; st < S; ++st) {
        const int64_t t = rev ? S - 1 - st : st;
        if (t >= len[b]) continue;
        const float* x = &X.f[xo(t, b)];
        for (int64_t j = 0; j < 4 * H; ++j) {  // rows of W / R: i | o | f | c
          double ax = 0, ah = 0;
          for (int64_t k = 0; k < I; ++k) ax += double(w[j * I + k]) * x[k];
          for (int64_t k = 0; k < H; ++k) ah += double(r[j * H + k]) * h[k];
          g[j] = ax + ah + bias[j] + bias[4 * H + j];
        }
        for (int64_t j = 0; j < H; ++j) {
          const float ig = sigmoid(float(g[j] + double(peep[j]) * c[j]));
          const float fg = sigmoid(float(g[2 * H + j] + double(peep[2 * H + j]) * c[j]));
          const float ct = std::tanh(float(g[3 * H + j]));
          const float cn = fg * c[j] + ig * ct;
          const float og = sigmoid(float(g[H + j] + double(peep[H + j]) * cn));
          c[j] = cn;
          h[j] = og * std::tanh(cn);
        }
        std::copy(h.begin(), h.end(), Y.f.begin() + yo(t, d, b));
      }
      std::copy(h.begin(), h.end(), Yh.f.begin() + ho(d, b));
      std::copy(c.begin(), c.end(), Yc.f.begin() + ho(d, b));
    }
  }
}

// ---- normalisations and activations of framework-exported MLPs (PyTorch / Keras): statistics
// and transcendental arguments in double, outputs float.

// BatchNormalization, inference form: X [N][C][...] with per-channel scale, B, mean, var.
Tensor batch_norm(const onnx::Node& n, const Tensor& X, const Tensor& scale, const Tensor& B, const Tensor& mean,
                  const Tensor& var) {
  if (n.geti("training_mode", 0) != 0)
    throw std::runtime_error("BatchNormalization: training_mode=1 is not supported (inference only)");
  if (X.dims.size() < 2) throw std::runtime_error("BatchNormalization: X must have a channel axis (rank >= 2)");
  const int64_t C = X.dims[1];
  for (const Tensor* t : {&scale, &B, &mean, &var})
    if (t->numel() != C) throw std::runtime_error("BatchNormalization: scale / B / mean / var must hold one value per channel");
  const double eps = n.getf("epsilon", 1e-5f);
  const auto x = as_float(X), s = as_float(scale), b = as_float(B), m = as_float(mean), v = as_float(var);
  int64_t inner = 1;
  for (size_t d = 2; d < X.dims.size(); ++d) inner *= X.dims[d];
  Tensor out = make(X.dims);
  for (int64_t e = 0; e < X.numel(); ++e) {
    const int64_t c = (e / inner) % C;
    out.f[e] = float((double(x[e]) - m[c]) / std::sqrt(double(v[c]) + eps) * s[c] + b[c]);
  }
  return out;
}

// LayerNormalization over the last axis: two passes (mean, then squared deviations) in double.
Tensor layer_norm(const onnx::Node& n, const Tensor& X, const Tensor& scale, const Tensor* B) {
  const int64_t rank = int64_t(X.dims.size());
  const int64_t axis = n.geti("axis", -1);
  if (rank < 1 || (axis != -1 && axis != rank - 1))
    throw std::runtime_error("LayerNormalization: axis " + std::to_string(axis) + " is not supported (last axis only)");
  const int64_t C = X.dims.back();
  if (scale.numel() != C) throw std::runtime_error("LayerNormalization: Scale must hold one value per column");
  if (B && B->numel() != C) throw std::runtime_error("LayerNormalization: B must hold one value per column");
  const double eps = n.getf("epsilon", 1e-5f);
  const auto x = as_float(X), s = as_float(scale);
  const std::vector<float> b = B ? as_float(*B) : std::vector<float>();
  Tensor out = make(X.dims);
  for (int64_t r = 0; r < X.numel() / std::max<int64_t>(C, 1); ++r) {
    const float* z = &x[r * C];
    double mu = 0, ss = 0;
    for (int64_t c = 0; c < C; ++c) mu += z[c];
    mu /= double(C);
    for (int64_t c = 0; c < C; ++c) ss += (z[c] - mu) * (z[c] - mu);
    const double inv = 1.0 / std::sqrt(ss / double(C) + eps);
    for (int64_t c = 0; c < C; ++c) out.f[r * C + c] = float((z[c] - mu) * inv * s[c] + (B ? double(b[c]) : 0.0));
  }
  return out;
}

inline float softplus(float x) { return float(std::max(double(x), 0.0) + std::log1p(std::exp(-std::fabs(double(x))))); }

float gelu(float xf, bool tanh_form) {
  const double x = xf;
  if (tanh_form) return float(0.5 * x * (1.0 + std::tanh(0.7978845608028654 * (x + 0.044715 * x * x * x))));
  return float(0.5 * x * (1.0 + std::erf(x * 0.7071067811865476)));
}

// ---- ai.onnx.ml linear models and preprocessing (sklearn-style pipelines: Scaler ->
// LinearClassifier -> ZipMap; Normalizer; LinearRegressor). Semantics follow the ai.onnx.ml
// operator definitions; ORT itself is not available offline, so exact ORT parity is unpinned
// (tests compare against numpy references of the definitions below).

int32_t post_code(const onnx::Node& n) {
  const std::string p = n.gets("post_transform", "NONE");
  if (p == "NONE") return trees::NONE;
  if (p == "LOGISTIC") return trees::LOGISTIC;
  if (p == "SOFTMAX") return trees::SOFTMAX;
  if (p == "SOFTMAX_ZERO") return trees::SOFTMAX_ZERO;
  if (p == "PROBIT") return trees::PROBIT;
  throw std::runtime_error(n.op_type + ": unknown post_transform " + p);
}

// one row of K scores through a post transform, in place
void post_row(int32_t post, float* z, int64_t k) {
  if (post == trees::LOGISTIC) {
    for (int64_t c = 0; c < k; ++c) z[c] = sigmoid(z[c]);
  } else if (post == trees::SOFTMAX || post == trees::SOFTMAX_ZERO) {
    const bool zero = post == trees::SOFTMAX_ZERO;
    float m = -INFINITY;
    for (int64_t c = 0; c < k; ++c) if (!(zero && z[c] == 0.f)) m = std::max(m, z[c]);
    double s = 0;
    for (int64_t c = 0; c < k; ++c) {
      if (zero && z[c] == 0.f) continue;
      z[c] = std::exp(z[c] - m);
      s += z[c];
    }
    for (int64_t c = 0; c < k; ++c) z[c] = (zero && z[c] == 0.f) || s <= 0 ? 0.f : float(z[c] / s);
  } else if (post == trees::PROBIT) {
    for (int64_t c = 0; c < k; ++c) z[c] = 1.41421356f * trees::erfinv(2 * z[c] - 1);
  }
}

// rows of X ([N][C], or one row [C]) times coefficient rows W [E][C] plus intercepts: [N][E]
std::vector<float> linear_rows(const std::string& op, const Tensor& X, const std::vector<float>& W,
                               const std::vector<float>& b, int64_t E, int64_t& N) {
  const auto x = as_float(X);
  const int64_t C = X.dims.empty() ? 1 : X.dims.back();
  N = X.dims.size() <= 1 ? 1 : X.numel() / std::max<int64_t>(C, 1);
  if (E < 1 || int64_t(W.size()) != E * C) throw std::runtime_error(op + ": coefficients do not match [E][C]");
  if (!b.empty() && int64_t(b.size()) != E) throw std::runtime_error(op + ": intercepts do not match E");
  std::vector<float> y(size_t(N * E));
  for (int64_t i = 0; i < N; ++i)
    for (int64_t e = 0; e < E; ++e) {
      double s = b.empty() ? 0.0 : double(b[e]);
      for (int64_t c = 0; c < C; ++c) s += double(W[e * C + c]) * double(x[i * C + c]);
      y[i * E + e] = float(s);
    }
  return y;
}

const std::vector<float>& attr_floats(const onnx::Node& n, const char* name) {
  static const std::vector<float> none;
  auto a = n.attr(name);
  return a ? a->floats : none;
}

// LinearClassifier: outputs (label [N] int64, scores [N][K]). One coefficient row is the binary
// case: raw score s becomes the two columns [-s, s] before the post transform (LOGISTIC then
// gives [sigmoid(-s), sigmoid(s)]) and the label is classlabels[s > 0]. E rows: label =
// classlabels[argmax raw]. String class labels yield the class index as the label.
void linear_classifier(const onnx::Node& n, const Tensor& X, Tensor& labels, Tensor& scores) {
  const auto& W = attr_floats(n, "coefficients");
  const auto& b = attr_floats(n, "intercepts");
  const int64_t C = X.dims.empty() ? 1 : X.dims.back();
  const int64_t E = !b.empty() ? int64_t(b.size()) : int64_t(W.size()) / std::max<int64_t>(C, 1);
  std::vector<int64_t> cl;
  if (auto a = n.attr("classlabels_ints")) cl = a->ints;
  else if (auto s = n.attr("classlabels_strings"))
    for (size_t k = 0; k < s->strings.size(); ++k) cl.push_back(int64_t(k));
  int64_t N = 0;
  auto raw = linear_rows(n.op_type, X, W, b, E, N);
  const int32_t post = post_code(n);
  const int64_t K = E == 1 ? 2 : E;
  labels = make({N}, INT64);
  scores = make({N, K});
  for (int64_t i = 0; i < N; ++i) {
    float* z = &scores.f[i * K];
    int64_t best = 0;
    if (E == 1) {
      z[0] = -raw[i];
      z[1] = raw[i];
      best = raw[i] > 0.f ? 1 : 0;
    } else {
      for (int64_t e = 0; e < E; ++e) {
        z[e] = raw[i * E + e];
        if (z[e] > z[best]) best = e;
      }
    }
    post_row(post, z, K);
    labels.i[i] = best < int64_t(cl.size()) ? cl[best] : best;
  }
}

}  // namespace

Executor::Executor(onnx::Model model) : model_(std::move(model)) {
  auto& g = model_.graph;
  std::set<std::string> avail;
  for (auto& kv : g.initializers) avail.insert(kv.first);
  for (auto& v : g.inputs) avail.insert(v.name);
  avail.insert("");
  std::vector<bool> done(g.nodes.size(), false);
  for (size_t pass = 0; pass < g.nodes.size(); ++pass) {
    bool progress = false;
    for (size_t k = 0; k < g.nodes.size(); ++k) {
      if (done[k]) continue;
      bool ready = true;
      for (auto& in : g.nodes[k].inputs) ready &= avail.count(in) > 0;
      if (!ready) continue;
      done[k] = true;
      progress = true;
      order_.push_back(k);
      for (auto& o : g.nodes[k].outputs) avail.insert(o);
    }
    if (!progress) break;
  }
  if (order_.size() != g.nodes.size()) throw std::runtime_error("onnx: graph has unresolvable inputs or a cycle");
  for (size_t k = 0; k < g.nodes.size(); ++k) {
    const auto& op = g.nodes[k].op_type;
    if (op == "TreeEnsembleClassifier" || op == "TreeEnsembleRegressor" || op == "TreeEnsemble")
      ensembles_[k] = std::make_shared<trees::Ensemble>(trees::compile(g.nodes[k]));
    else if (op == "SVMClassifier" || op == "SVMRegressor")
      svms_[k] = std::make_shared<svm::SvmModel>(svm::compile(g.nodes[k]));
  }
}

const svm::SvmModel* Executor::svm_model(size_t node_index) const {
  auto it = svms_.find(node_index);
  return it == svms_.end() ? nullptr : it->second.get();
}

const trees::Ensemble* Executor::ensemble(size_t node_index) const {
  auto it = ensembles_.find(node_index);
  return it == ensembles_.end() ? nullptr : it->second.get();
}

std::map<std::string, Tensor> Executor::run(const std::map<std::string, Tensor>& inputs) const {
  const auto& g = model_.graph;
  std::map<std::string, Tensor> vals;
  for (auto& kv : g.initializers) vals[kv.first] = kv.second;
  for (auto& v : g.inputs) {
    auto it = inputs.find(v.name);
    if (it == inputs.end()) throw std::runtime_error("executor: missing input " + v.name);
    vals[v.name] = it->second;
  }
  auto get = [&](const std::string& name) -> const Tensor& {
    auto it = vals.find(name);
    if (it == vals.end()) throw std::runtime_error("executor: value not computed: " + name);
    return it->second;
  };
  auto opt = [&](const onnx::Node& n, size_t i) -> const Tensor* {
    if (i >= n.inputs.size() || n.inputs[i].empty()) return nullptr;
    return &get(n.inputs[i]);
  };
  auto is_read = [&](const std::string& name) {  // by a node or as a graph output
    for (auto& m : g.nodes)
      if (std::find(m.inputs.begin(), m.inputs.end(), name) != m.inputs.end()) return true;
    for (auto& v : g.outputs)
      if (v.name == name) return true;
    return false;
  };
  for (size_t k : order_) {
    const auto& n = g.nodes[k];
    const std::string& op = n.op_type;
    Tensor out;
    if (op == "Gemm") out = gemm(n, get(n.inputs[0]), get(n.inputs[1]), opt(n, 2));
    else if (op == "MatMul") out = matmul(get(n.inputs[0]), get(n.inputs[1]));
    else if (op == "Add") out = binary(get(n.inputs[0]), get(n.inputs[1]), [](float a, float b) { return a + b; });
    else if (op == "Sub") out = binary(get(n.inputs[0]), get(n.inputs[1]), [](float a, float b) { return a - b; });
    else if (op == "Mul") out = binary(get(n.inputs[0]), get(n.inputs[1]), [](float a, float b) { return a * b; });
    else if (op == "Div") out = binary(get(n.inputs[0]), get(n.inputs[1]), [](float a, float b) { return a / b; });
    else if (op == "Max") out = binary(get(n.inputs[0]), get(n.inputs[1]), [](float a, float b) { return std::max(a, b); });
    else if (op == "Min") out = binary(get(n.inputs[0]), get(n.inputs[1]), [](float a, float b) { return std::min(a, b); });
    else if (op == "Relu") out = unary(get(n.inputs[0]), [](float x) { return x > 0 ? x : 0.f; });
    else if (op == "LeakyRelu") { float a = n.getf("alpha", 0.01f); out = unary(get(n.inputs[0]), [a](float x) { return x > 0 ? x : a * x; }); }
    else if (op == "Sigmoid") out = unary(get(n.inputs[0]), sigmoid);
    else if (op == "Tanh") out = unary(get(n.inputs[0]), [](float x) { return std::tanh(x); });
    else if (op == "Exp") out = unary(get(n.inputs[0]), [](float x) { return std::exp(x); });
    else if (op == "Log") out = unary(get(n.inputs[0]), [](float x) { return std::log(x); });
    else if (op == "Abs") out = unary(get(n.inputs[0]), [](float x) { return std::fabs(x); });
    else if (op == "Neg") out = unary(get(n.inputs[0]), [](float x) { return -x; });
    else if (op == "Sqrt") out = unary(get(n.inputs[0]), [](float x) { return std::sqrt(x); });
    else if (op == "Identity") out = get(n.inputs[0]);
    else if (op == "Clip") {
      float lo = -INFINITY, hi = INFINITY;
      if (auto t = opt(n, 1)) lo = as_float(*t)[0];
      if (auto t = opt(n, 2)) hi = as_float(*t)[0];
      if (n.attr("min")) lo = n.getf("min", lo);
      if (n.attr("max")) hi = n.getf("max", hi);
      out = unary(get(n.inputs[0]), [lo, hi](float x) { return std::min(std::max(x, lo), hi); });
    } else if (op == "Elu") {
      const double a = n.getf("alpha", 1.f);
      out = unary(get(n.inputs[0]), [a](float x) { return x > 0 ? x : float(a * std::expm1(double(x))); });
    } else if (op == "Selu") {
      const double a = n.getf("alpha", 1.67326319217681884765625f), g2 = n.getf("gamma", 1.05070102214813232421875f);
      out = unary(get(n.inputs[0]), [a, g2](float x) { return float(x > 0 ? g2 * x : g2 * a * std::expm1(double(x))); });
    } else if (op == "Softplus") {
      out = unary(get(n.inputs[0]), softplus);
    } else if (op == "HardSigmoid") {
      const double a = n.getf("alpha", 0.2f), b = n.getf("beta", 0.5f);
      out = unary(get(n.inputs[0]), [a, b](float x) { return float(std::min(1.0, std::max(0.0, a * x + b))); });
    } else if (op == "Gelu") {
      const std::string ap = n.gets("approximate", "none");
      if (ap != "none" && ap != "tanh") throw std::runtime_error("Gelu: approximate must be none or tanh, got " + ap);
      const bool th = ap == "tanh";
      out = unary(get(n.inputs[0]), [th](float x) { return gelu(x, th); });
    } else if (op == "PRelu") {
      if (n.inputs.size() < 2) throw std::runtime_error("PRelu: needs X and slope");
      const Tensor& x = get(n.inputs[0]);
      const Tensor& sl = get(n.inputs[1]);
      const int64_t C = x.dims.empty() ? 1 : x.dims.back();
      if (sl.numel() != 1 && (sl.numel() != C || (!sl.dims.empty() && sl.dims.back() != C)))
        throw std::runtime_error("PRelu: slope must be a scalar or one value per column");
      const auto s = as_float(sl), xf = as_float(x);
      out = make(x.dims);
      for (int64_t e = 0; e < x.numel(); ++e) out.f[e] = xf[e] >= 0 ? xf[e] : s[s.size() == 1 ? 0 : e % C] * xf[e];
    } else if (op == "BatchNormalization") {
      if (n.inputs.size() < 5) throw std::runtime_error("BatchNormalization: needs X, scale, B, mean and var");
      out = batch_norm(n, get(n.inputs[0]), get(n.inputs[1]), get(n.inputs[2]), get(n.inputs[3]), get(n.inputs[4]));
    } else if (op == "LayerNormalization") {
      if (n.inputs.size() < 2 || n.inputs[1].empty()) throw std::runtime_error("LayerNormalization: Scale is required");
      for (size_t o = 1; o < n.outputs.size(); ++o)
        if (!n.outputs[o].empty() && is_read(n.outputs[o]))
          throw std::runtime_error("LayerNormalization: the Mean / InvStdDev outputs are not produced");
      out = layer_norm(n, get(n.inputs[0]), get(n.inputs[1]), opt(n, 2));
    } else if (op == "Dropout") {
      // inference: the identity; a constant true training_mode would make it random
      if (n.inputs.size() > 2 && !n.inputs[2].empty()) {
        auto it = g.initializers.find(n.inputs[2]);
        if (it != g.initializers.end() && it->second.numel() > 0 && as_int(it->second)[0] != 0)
          throw std::runtime_error("Dropout: training_mode is a constant true (inference only)");
      }
      out = get(n.inputs[0]);
      if (n.outputs.size() > 1 && !n.outputs[1].empty() && is_read(n.outputs[1])) {
        Tensor mask = make(out.dims);
        std::fill(mask.f.begin(), mask.f.end(), 1.f);
        vals[n.outputs[1]] = std::move(mask);
      }
    } else if (op == "Cast") {
      int64_t to = n.geti("to", FLOAT);
      const Tensor& x = get(n.inputs[0]);
      out.dims = x.dims;
      if (to == INT64 || to == onnx::INT32) { out.dtype = INT64; out.i = as_int(x); }
      else { out.dtype = FLOAT; out.f = as_float(x); }
    } else if (op == "Softmax") {
      const Tensor& x = get(n.inputs[0]);
      int64_t ax = norm_axis(n.geti("axis", -1), x.dims.size());
      int64_t inner = 1;
      for (size_t d = ax + 1; d < x.dims.size(); ++d) inner *= x.dims[d];
      int64_t len = x.dims[ax], outer = x.numel() / (len * inner);
      out = make(x.dims);
      for (int64_t o = 0; o < outer; ++o)
        for (int64_t i = 0; i < inner; ++i) {
          float m = -INFINITY;
          for (int64_t l = 0; l < len; ++l) m = std::max(m, x.f[(o * len + l) * inner + i]);
          double s = 0;
          for (int64_t l = 0; l < len; ++l) s += std::exp(double(x.f[(o * len + l) * inner + i] - m));
          for (int64_t l = 0; l < len; ++l)
            out.f[(o * len + l) * inner + i] = float(std::exp(double(x.f[(o * len + l) * inner + i] - m)) / s);
        }
    } else if (op == "Flatten") {
      const Tensor& x = get(n.inputs[0]);
      int64_t ax = norm_axis(n.geti("axis", 1), x.dims.size());
      int64_t a = 1;
      for (int64_t d = 0; d < ax; ++d) a *= x.dims[d];
      out = x;
      out.dims = {a, x.numel() / std::max<int64_t>(a, 1)};
    } else if (op == "Reshape") {
      const Tensor& x = get(n.inputs[0]);
      auto shp = as_int(get(n.inputs[1]));
      int64_t known = 1, neg = -1;
      for (size_t d = 0; d < shp.size(); ++d) {
        if (shp[d] == 0) shp[d] = x.dims.at(d);
        if (shp[d] == -1) neg = int64_t(d); else known *= shp[d];
      }
      if (neg >= 0) shp[neg] = x.numel() / known;
      out = x;
      out.dims = shp;
      if (out.numel() != x.numel()) throw std::runtime_error("Reshape: element count mismatch");
    } else if (op == "Squeeze" || op == "Unsqueeze") {
      const Tensor& x = get(n.inputs[0]);
      std::vector<int64_t> axes;
      if (auto t = opt(n, 1)) axes = as_int(*t);
      else if (auto a = n.attr("axes")) axes = a->ints;
      out = x;
      if (op == "Squeeze") {
        std::vector<int64_t> d;
        for (size_t k2 = 0; k2 < x.dims.size(); ++k2) {
          bool drop = axes.empty() ? x.dims[k2] == 1 : false;
          for (auto a : axes) drop |= norm_axis(a, x.dims.size()) == int64_t(k2);
          if (!drop) d.push_back(x.dims[k2]);
        }
        out.dims = d;
      } else {
        size_t r = x.dims.size() + axes.size();
        std::vector<int64_t> d;
        std::set<int64_t> ax;
        for (auto a : axes) ax.insert(a < 0 ? a + int64_t(r) : a);
        size_t src = 0;
        for (size_t k2 = 0; k2 < r; ++k2) d.push_back(ax.count(k2) ? 1 : x.dims[src++]);
        out.dims = d;
      }
    } else if (op == "Concat") {
      std::vector<const Tensor*> ts;
      for (auto& in : n.inputs) ts.push_back(&get(in));
      int64_t ax = norm_axis(n.geti("axis", 0), ts[0]->dims.size());
      std::vector<int64_t> d = ts[0]->dims;
      d[ax] = 0;
      for (auto t : ts) d[ax] += t->dims[ax];
      out = make(d);
      int64_t outer = 1, inner = 1;
      for (int64_t k2 = 0; k2 < ax; ++k2) outer *= d[k2];
      for (size_t k2 = ax + 1; k2 < d.size(); ++k2) inner *= d[k2];
      int64_t off = 0;
      for (auto t : ts) {
        auto tf = as_float(*t);
        int64_t len = t->dims[ax];
        for (int64_t o = 0; o < outer; ++o)
          std::copy(tf.begin() + o * len * inner, tf.begin() + (o + 1) * len * inner,
                    out.f.begin() + (o * d[ax] + off) * inner);
        off += len;
      }
    } else if (op == "Transpose") {
      const Tensor& x = get(n.inputs[0]);
      size_t r = x.dims.size();
      std::vector<int64_t> perm(r);
      if (auto a = n.attr("perm")) perm = a->ints;
      else for (size_t k2 = 0; k2 < r; ++k2) perm[k2] = int64_t(r - 1 - k2);
      std::vector<int64_t> d(r), st(r, 1);
      for (int k2 = int(r) - 2; k2 >= 0; --k2) st[k2] = st[k2 + 1] * x.dims[k2 + 1];
      for (size_t k2 = 0; k2 < r; ++k2) d[k2] = x.dims[perm[k2]];
      out = make(d);
      std::vector<int64_t> idx(r, 0);
      for (int64_t e = 0; e < out.numel(); ++e) {
        int64_t src = 0;
        for (size_t k2 = 0; k2 < r; ++k2) src += idx[k2] * st[perm[k2]];
        out.f[e] = x.f[src];
        for (int k2 = int(r) - 1; k2 >= 0; --k2) { if (++idx[k2] < d[k2]) break; idx[k2] = 0; }
      }
    } else if (op == "TreeEnsembleClassifier" || op == "TreeEnsembleRegressor" || op == "TreeEnsemble") {
      const auto* e = ensemble(k);
      const Tensor& x = get(n.inputs[0]);
      auto xf = as_float(x);
      int64_t N = x.dims.size() == 1 ? 1 : x.dims[0];
      int64_t F = x.numel() / std::max<int64_t>(N, 1);
      std::vector<float> sc(size_t(N) * e->n_targets);
      trees::eval_raw(*e, xf.data(), N, F, sc.data());
      Tensor probs = make({N, e->n_outputs});
      if (e->classifier) {
        Tensor labels = make({N}, INT64);
        trees::post_transform(*e, sc.data(), N, probs.f.data(), labels.i.data());
        vals[n.outputs[0]] = labels;
        if (n.outputs.size() > 1) vals[n.outputs[1]] = probs;
      } else {
        trees::post_transform(*e, sc.data(), N, probs.f.data(), nullptr);
        vals[n.outputs[0]] = probs;
      }
      continue;
    } else if (op == "LinearClassifier") {
      Tensor labels, scores;
      linear_classifier(n, get(n.inputs[0]), labels, scores);
      vals[n.outputs[0]] = std::move(labels);
      if (n.outputs.size() > 1) vals[n.outputs[1]] = std::move(scores);
      continue;
    } else if (op == "SVMClassifier" || op == "SVMRegressor") {
      const svm::SvmModel& m = *svm_model(k);
      const Tensor& x = get(n.inputs[0]);
      const auto xf = as_float(x);
      const int64_t C = x.dims.empty() ? 1 : x.dims.back();
      const int64_t N = x.dims.size() <= 1 ? 1 : x.numel() / std::max<int64_t>(C, 1);
      std::vector<float> dec(size_t(N), 0.f);
      svm::decision(m, xf.data(), N, C, dec.data());
      if (!m.classifier) {
        out = make({N, 1});
        for (int64_t i = 0; i < N; ++i) {
          out.f[i] = m.one_class ? (dec[i] > 0.f ? 1.f : -1.f) : dec[i];
          post_row(m.post, &out.f[i], 1);
        }
      } else {
        // outputs as LinearClassifier writes them: label [N] int64, scores [N][2]
        Tensor labels = make({N}, INT64), scores = make({N, 2});
        for (int64_t i = 0; i < N; ++i) {
          float* z = &scores.f[i * 2];
          int64_t best;
          if (m.platt) {
            z[0] = 1.f / (1.f + std::exp(m.prob_a * dec[i] + m.prob_b));
            z[1] = 1.f - z[0];
            best = z[1] > z[0] ? 1 : 0;
          } else {
            z[0] = dec[i];
            z[1] = -dec[i];
            best = dec[i] > 0.f ? 0 : 1;
            post_row(m.post, z, 2);
          }
          labels.i[i] = m.classlabels[best];
        }
        vals[n.outputs[0]] = std::move(labels);
        if (n.outputs.size() > 1) vals[n.outputs[1]] = std::move(scores);
        continue;
      }
    } else if (op == "LinearRegressor") {
      const Tensor& x = get(n.inputs[0]);
      const int64_t E = n.geti("targets", 1);
      int64_t N = 0;
      auto y = linear_rows(op, x, attr_floats(n, "coefficients"), attr_floats(n, "intercepts"), E, N);
      const int32_t post = post_code(n);
      out = make({N, E});
      out.f = std::move(y);
      for (int64_t i = 0; i < N; ++i) post_row(post, &out.f[i * E], E);
    } else if (op == "Scaler") {
      // Y = (X - offset) * scale, offset / scale per column (or one value for all)
      const Tensor& x = get(n.inputs[0]);
      const auto& off = attr_floats(n, "offset");
      const auto& sc = attr_floats(n, "scale");
      const int64_t C = x.dims.empty() ? 1 : x.dims.back();
      auto ok = [C](size_t s) { return s == 0 || s == 1 || int64_t(s) == C; };
      if (!ok(off.size()) || !ok(sc.size())) throw std::runtime_error("Scaler: offset / scale length must be 1 or C");
      auto xf = as_float(x);
      out = make(x.dims);
      for (int64_t e = 0; e < x.numel(); ++e) {
        const int64_t c = e % C;
        const float o = off.empty() ? 0.f : off[off.size() == 1 ? 0 : c];
        const float s = sc.empty() ? 1.f : sc[sc.size() == 1 ? 0 : c];
        out.f[e] = (xf[e] - o) * s;
      }
    } else if (op == "Imputer") {
      out = cols::imputer(n, get(n.inputs.at(0)));
    } else if (op == "Binarizer") {
      out = cols::binarizer(n, get(n.inputs.at(0)));
    } else if (op == "OneHotEncoder") {
      out = cols::one_hot_encoder(n, get(n.inputs.at(0)));
    } else if (op == "ArrayFeatureExtractor" || op == "Gather") {
      if (n.inputs.empty()) throw std::runtime_error(op + ": needs a value and its indices");
      const bool cst = n.inputs.size() > 1 && g.initializers.count(n.inputs[1]) > 0;
      out = op == "Gather" ? cols::gather(n, get(n.inputs[0]), opt(n, 1), cst)
                           : cols::array_feature_extractor(n, get(n.inputs[0]), opt(n, 1), cst);
    } else if (op == "Slice") {
      if (n.inputs.empty()) throw std::runtime_error("Slice: needs data, starts and ends");
      bool cst = true;
      for (size_t i = 1; i < n.inputs.size(); ++i) cst &= n.inputs[i].empty() || g.initializers.count(n.inputs[i]) > 0;
      out = cols::slice(n, get(n.inputs[0]), opt(n, 1), opt(n, 2), opt(n, 3), opt(n, 4), cst);
    } else if (op == "Conv") {
      if (n.inputs.size() < 2) throw std::runtime_error("Conv: needs X and W");
      out = conv::conv1d(n, get(n.inputs[0]), get(n.inputs[1]), g.initializers.count(n.inputs[1]) > 0, opt(n, 2));
    } else if (op == "Pad") {
      if (n.inputs.empty()) throw std::runtime_error("Pad: needs data");
      bool cst = true;
      for (size_t i = 1; i < n.inputs.size() && i < 3; ++i) cst &= n.inputs[i].empty() || g.initializers.count(n.inputs[i]) > 0;
      out = conv::pad(n, get(n.inputs[0]), opt(n, 1), opt(n, 2), cst, opt(n, 3) != nullptr);
    } else if (op == "GlobalAveragePool" || op == "GlobalMaxPool") {
      out = conv::global_pool(op.c_str(), get(n.inputs.at(0)));
    } else if (op == "ReduceMean" || op == "ReduceMax" || op == "ReduceSum") {
      out = conv::reduce(n, get(n.inputs.at(0)), opt(n, 1), n.inputs.size() > 1 && g.initializers.count(n.inputs[1]) > 0);
    } else if (op == "FeatureVectorizer") {
      std::vector<const Tensor*> ts;
      for (auto& in : n.inputs) ts.push_back(&get(in));
      out = cols::feature_vectorizer(n, ts);
    } else if (op == "Normalizer") {
      // per row (last axis): MAX divides by the row maximum, L1 by sum |x|, L2 by sqrt(sum x^2);
      // a zero denominator leaves the row unchanged
      const Tensor& x = get(n.inputs[0]);
      const std::string norm = n.gets("norm", "MAX");
      if (norm != "MAX" && norm != "L1" && norm != "L2") throw std::runtime_error("Normalizer: norm " + norm);
      const int64_t C = x.dims.empty() ? 1 : x.dims.back();
      out = make(x.dims);
      out.f = as_float(x);
      for (int64_t r = 0; r < x.numel() / std::max<int64_t>(C, 1); ++r) {
        float* z = &out.f[r * C];
        double d = norm == "MAX" ? -INFINITY : 0.0;
        for (int64_t c = 0; c < C; ++c)
          d = norm == "MAX" ? std::max(d, double(z[c])) : norm == "L1" ? d + std::fabs(double(z[c]))
                                                                        : d + double(z[c]) * z[c];
        if (norm == "L2") d = std::sqrt(d);
        if (d != 0.0 && std::isfinite(d))
          for (int64_t c = 0; c < C; ++c) z[c] = float(double(z[c]) / d);
      }
    } else if (op == "ZipMap") {
      // seq(map(label -> probability)) is represented densely: the [N][K] probability tensor,
      // columns in classlabels order (what every consumer of the model output reads)
      const Tensor& x = get(n.inputs[0]);
      out = make(x.dims);
      out.f = as_float(x);
    } else if (op == "QuantizeLinear" || op == "DequantizeLinear") {
      if (n.inputs.size() < 2) throw std::runtime_error(op + ": needs a value and a scale");
      for (size_t i = 1; i < n.inputs.size() && i < 3; ++i)
        if (!n.inputs[i].empty() && !g.initializers.count(n.inputs[i]))
          throw std::runtime_error(op + ": scale and zero point must be constants (initializers)");
      out = op == "QuantizeLinear" ? quantize_linear(n, get(n.inputs[0]), get(n.inputs[1]), opt(n, 2))
                                   : dequantize_linear(n, get(n.inputs[0]), get(n.inputs[1]), opt(n, 2));
    } else if (op == "QLinearMatMul" || op == "QLinearConv" || op == "QLinearAdd" || op == "QGemm" ||
               op == "MatMulInteger" || op == "ConvInteger" || op == "DynamicQuantizeLinear") {
      throw std::runtime_error("executor: " + op + kQdqOnly);
    } else if (op == "GRU") {
      Tensor Y, Yh;
      gru(n, get(n.inputs[0]), get(n.inputs[1]), get(n.inputs[2]), opt(n, 3), opt(n, 4),
          opt(n, 5), Y, Yh);
      if (!n.outputs.empty() && !n.outputs[0].empty()) vals[n.outputs[0]] = Y;
      if (n.outputs.size() > 1 && !n.outputs[1].empty()) vals[n.outputs[1]] = Yh;
      continue;
    } else if (op == "LSTM") {
      // inputs: X, W, R, B, sequence_lens, initial_h, initial_c, P; outputs: Y, Y_h, Y_c
      if (n.inputs.size() < 3) throw std::runtime_error("LSTM: needs X, W and R");
      Tensor Y, Yh, Yc;
      lstm(n, get(n.inputs[0]), get(n.inputs[1]), get(n.inputs[2]), opt(n, 3), opt(n, 4), opt(n, 5), opt(n, 6),
           opt(n, 7), Y, Yh, Yc);
      if (!n.outputs.empty() && !n.outputs[0].empty()) vals[n.outputs[0]] = Y;
      if (n.outputs.size() > 1 && !n.outputs[1].empty()) vals[n.outputs[1]] = Yh;
      if (n.outputs.size() > 2 && !n.outputs[2].empty()) vals[n.outputs[2]] = Yc;
      continue;
    } else {
      throw std::runtime_error("executor: unsupported op " + op + " (node " + n.name + ")");
    }
    vals[n.outputs[0]] = std::move(out);
  }
  std::map<std::string, Tensor> res;
  for (auto& v : g.outputs) res[v.name] = get(v.name);
  return res;
}

}  // namespace igp::exec
