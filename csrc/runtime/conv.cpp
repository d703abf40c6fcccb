#include "conv.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>

namespace igp::conv {
namespace {

using onnx::FLOAT;

[[noreturn]] void fail(const char* op, const std::string& what) { throw std::runtime_error(std::string(op) + ": " + what); }

const Tensor& float_in(const char* op, const char* which, const Tensor& x) {
  if (x.dtype != FLOAT || int64_t(x.f.size()) != x.numel()) fail(op, std::string(which) + " must be a float tensor");
  return x;
}

Tensor make(std::vector<int64_t> dims) {
  Tensor t;
  t.dtype = FLOAT;
  t.dims = std::move(dims);
  t.f.assign(size_t(t.numel()), 0.f);
  return t;
}

// max with the NaN rule of this file: a NaN among the elements gives NaN
inline float nan_max(float m, float v) { return std::isnan(m) ? m : (std::isnan(v) || v > m) ? v : m; }

const int64_t kMaxDim = int64_t(1) << 31;   // padded extents stay inside what the loops index

}  // namespace

Tensor conv1d(const Node& n, const Tensor& x, const Tensor& w, bool w_const, const Tensor* b) {
  const char* op = "Conv";
  if (!w_const) fail(op, "W must be a constant (an initializer)");
  float_in(op, "X", x);
  float_in(op, "W", w);
  if (w.dims.size() != 3) fail(op, "only 1-D convolutions are supported (W [M][C][k]; this one has rank " + std::to_string(w.dims.size()) + ")");
  if (x.dims.size() != 3) fail(op, "X must be [N][C][L] (rank " + std::to_string(x.dims.size()) + ")");
  const int64_t N = x.dims[0], C = x.dims[1], L = x.dims[2], M = w.dims[0], k = w.dims[2];
  if (n.geti("group", 1) != 1) fail(op, "group " + std::to_string(n.geti("group", 1)) + " is not supported (1 only)");
  if (const auto* a = n.attr("kernel_shape")) {
    if (a->ints.size() != 1) fail(op, "only 1-D convolutions are supported (kernel_shape has " + std::to_string(a->ints.size()) + " axes)");
    if (a->ints[0] != k) fail(op, "kernel_shape " + std::to_string(a->ints[0]) + " differs from W's kernel axis " + std::to_string(k));
  }
  if (k < 1) fail(op, "a kernel size of 0");
  if (M < 1 || w.dims[1] != C) fail(op, "W [" + std::to_string(M) + "][" + std::to_string(w.dims[1]) + "][k] does not match X's " + std::to_string(C) + " channels");
  int64_t d = 1;
  if (const auto* a = n.attr("dilations")) {
    if (a->ints.size() != 1) fail(op, "dilations must hold one value (1-D)");
    d = a->ints[0];
  }
  if (d < 1) fail(op, "a dilation of " + std::to_string(d));
  if (const auto* a = n.attr("strides")) {
    if (a->ints.size() != 1) fail(op, "strides must hold one value (1-D)");
    if (a->ints[0] != 1) fail(op, "stride " + std::to_string(a->ints[0]) + " is not supported (1 only)");
  }
  if (b) {
    float_in(op, "B", *b);
    if (b->numel() != M) fail(op, "B holds " + std::to_string(b->numel()) + " values for " + std::to_string(M) + " output channels");
  }
  if (d > kMaxDim / k) fail(op, "dilation x kernel size out of range");
  const int64_t span = d * (k - 1);
  int64_t pl = 0, pr = 0;
  const std::string ap = n.gets("auto_pad", "NOTSET");
  if (ap == "NOTSET") {
    if (const auto* a = n.attr("pads")) {
      if (a->ints.size() != 2) fail(op, "pads must hold 2 values [begin, end], not " + std::to_string(a->ints.size()));
      pl = a->ints[0];
      pr = a->ints[1];
    }
    if (pl < 0 || pr < 0) fail(op, "negative pads");
    if (pl > kMaxDim || pr > kMaxDim) fail(op, "pads out of range");
  } else if (ap == "SAME_UPPER" || ap == "SAME_LOWER") {
    pl = ap == "SAME_UPPER" ? span / 2 : span - span / 2;
    pr = span - pl;
  } else if (ap != "VALID") {
    fail(op, "unknown auto_pad " + ap);
  }
  const int64_t Lo = L + pl + pr - span;
  if (Lo < 1 && N * M > 0) fail(op, "the dilated kernel (" + std::to_string(span + 1) + " steps) does not fit the padded length " + std::to_string(L + pl + pr));
  Tensor y = make({N, M, std::max<int64_t>(Lo, 0)});
  for (int64_t i = 0; i < N; ++i)
    for (int64_t m = 0; m < M; ++m)
      for (int64_t t = 0; t < Lo; ++t) {
        double s = b ? double(b->f[m]) : 0.0;
        for (int64_t c = 0; c < C; ++c) {
          const float* xr = &x.f[(i * C + c) * L];
          const float* wr = &w.f[(m * C + c) * k];
          for (int64_t j = 0; j < k; ++j) {
            const int64_t p = t - pl + j * d;
            if (p >= 0 && p < L) s += double(wr[j]) * double(xr[p]);
          }
        }
        y.f[(i * M + m) * Lo + t] = float(s);
      }
  return y;
}

Tensor pad(const Node& n, const Tensor& x, const Tensor* pads_t, const Tensor* value_t, bool all_const, bool has_axes) {
  const char* op = "Pad";
  float_in(op, "the input", x);
  if (n.gets("mode", "constant") != "constant") fail(op, "mode " + n.gets("mode", "") + " is not supported (constant only)");
  if (has_axes) fail(op, "the axes input (opset 18) is not supported");
  std::vector<int64_t> pads;
  float value = 0.f;
  if (pads_t) {
    if (!all_const) fail(op, "pads and the value must be constants (initializers)");
    if (pads_t->dtype == FLOAT) fail(op, "pads must be an integer tensor");
    pads = pads_t->i;
    if (value_t) {
      if (value_t->numel() != 1) fail(op, "the value must be a scalar");
      value = value_t->dtype == FLOAT ? value_t->f[0] : float(value_t->i[0]);
    }
  } else if (const auto* a = n.attr("pads")) {   // opset 2: attributes (opset 1 called it paddings)
    pads = a->ints;
    value = n.getf("value", 0.f);
  } else {
    fail(op, "pads are missing");
  }
  const size_t r = x.dims.size();
  if (pads.size() != 2 * r) fail(op, std::to_string(pads.size()) + " pads for a value of rank " + std::to_string(r) + " (2 per axis)");
  std::vector<int64_t> od(r);
  for (size_t a = 0; a < r; ++a) {
    if (pads[a] < 0 || pads[r + a] < 0) fail(op, "negative pads");
    if (pads[a] > kMaxDim || pads[r + a] > kMaxDim) fail(op, "pads out of range");
    od[a] = x.dims[a] + pads[a] + pads[r + a];
  }
  int64_t total = 1;
  for (size_t a = 0; a < r; ++a) {
    if (od[a] > 0 && total > kMaxDim / od[a]) fail(op, "the padded tensor is too large");
    total *= od[a];
  }
  Tensor y = make(od);
  std::fill(y.f.begin(), y.f.end(), value);
  if (x.numel() == 0) return y;
  std::vector<int64_t> idx(r, 0);
  for (int64_t e = 0; e < x.numel(); ++e) {
    int64_t o = 0;
    for (size_t a = 0; a < r; ++a) o = o * od[a] + idx[a] + pads[a];
    y.f[o] = x.f[e];
    for (int a = int(r) - 1; a >= 0; --a) {
      if (++idx[a] < x.dims[a]) break;
      idx[a] = 0;
    }
  }
  return y;
}

Tensor global_pool(const char* op, const Tensor& x) {
  float_in(op, "the input", x);
  if (x.dims.size() < 3) fail(op, "the input must be [N][C][d...] (rank >= 3)");
  const bool is_max = std::string(op) == "GlobalMaxPool";
  const int64_t outer = x.dims[0] * x.dims[1];
  const int64_t inner = outer ? x.numel() / outer : 0;
  if (outer && inner < 1) fail(op, "nothing to pool (an empty spatial axis)");
  std::vector<int64_t> od(x.dims.size(), 1);
  od[0] = x.dims[0];
  od[1] = x.dims[1];
  Tensor y = make(od);
  for (int64_t o = 0; o < outer; ++o) {
    const float* p = &x.f[o * inner];
    if (is_max) {
      float m = p[0];
      for (int64_t e = 1; e < inner; ++e) m = nan_max(m, p[e]);
      y.f[o] = m;
    } else {
      double s = 0;
      for (int64_t e = 0; e < inner; ++e) s += double(p[e]);
      y.f[o] = float(s / double(inner));
    }
  }
  return y;
}

Tensor reduce(const Node& n, const Tensor& x, const Tensor* axes_t, bool axes_const) {
  const std::string ops = n.op_type;
  const char* op = ops.c_str();
  float_in(op, "the input", x);
  const int64_t r = int64_t(x.dims.size());
  std::vector<int64_t> axes;
  if (axes_t) {
    if (!axes_const) fail(op, "axes must be a constant (an initializer)");
    if (axes_t->dtype == FLOAT) fail(op, "axes must be an integer tensor");
    axes = axes_t->i;
  } else if (const auto* a = n.attr("axes")) {
    axes = a->ints;
  }
  std::vector<bool> red(size_t(r), false);
  if (axes.empty()) {
    if (n.geti("noop_with_empty_axes", 0) != 0) return x;
    std::fill(red.begin(), red.end(), true);
  }
  for (int64_t a : axes) {
    if (a < -r || a >= r) fail(op, "axis " + std::to_string(a) + " out of range for rank " + std::to_string(r));
    red[size_t(a < 0 ? a + r : a)] = true;
  }
  const bool keep = n.geti("keepdims", 1) != 0;
  const bool is_max = ops == "ReduceMax", is_mean = ops == "ReduceMean";
  std::vector<int64_t> od;
  int64_t count = 1;
  for (int64_t a = 0; a < r; ++a) {
    if (red[a]) {
      count *= x.dims[a];
      if (keep) od.push_back(1);
    } else {
      od.push_back(x.dims[a]);
    }
  }
  Tensor y = make(od);
  if (y.numel() == 0) return y;
  if (count < 1 && (is_max || is_mean)) fail(op, "nothing to reduce (an empty axis)");
  // strides of the output laid over the input's axes (0 on a reduced axis)
  std::vector<int64_t> os(size_t(r), 0);
  int64_t m = 1;
  for (int64_t a = r - 1; a >= 0; --a)
    if (!red[a]) {
      os[a] = m;
      m *= x.dims[a];
    }
  std::vector<double> acc(size_t(y.numel()), 0.0);
  std::vector<char> seen(size_t(y.numel()), 0);
  std::vector<int64_t> idx(size_t(r), 0);
  for (int64_t e = 0; e < x.numel(); ++e) {   // ascending input order: one fixed order per output element
    int64_t o = 0;
    for (int64_t a = 0; a < r; ++a) o += idx[a] * os[a];
    if (is_max) {
      y.f[o] = seen[o] ? nan_max(y.f[o], x.f[e]) : x.f[e];
      seen[o] = 1;
    } else {
      acc[o] += double(x.f[e]);
    }
    for (int64_t a = r - 1; a >= 0; --a) {
      if (++idx[a] < x.dims[a]) break;
      idx[a] = 0;
    }
  }
  if (!is_max)
    for (int64_t o = 0; o < y.numel(); ++o) y.f[o] = float(is_mean ? acc[o] / double(count) : acc[o]);
  return y;
}

}  // namespace igp::conv
