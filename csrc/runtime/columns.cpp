#include "columns.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>

namespace igp::cols {
namespace {

using onnx::FLOAT;

[[noreturn]] void fail(const char* op, const std::string& what) { throw std::runtime_error(std::string(op) + ": " + what); }

// rows and columns of a value read as [N][C]: the last axis is the columns
void rows_cols(const char* op, const Tensor& x, int64_t& N, int64_t& C) {
  if (x.dims.empty()) fail(op, "the input must have a feature axis (rank >= 1)");
  C = x.dims.back();
  N = 1;
  for (size_t d = 0; d + 1 < x.dims.size(); ++d) N *= x.dims[d];
}

const Tensor& float_in(const char* op, const Tensor& x) {
  if (x.dtype != FLOAT) fail(op, "the input must be a float tensor");
  return x;
}

// constant integer tensor (int32 initializers arrive widened to int64 payloads)
const std::vector<int64_t>& int_const(const char* op, const char* what, const Tensor* t, bool is_const) {
  if (!t) fail(op, std::string(what) + " is missing");
  if (!is_const) fail(op, std::string(what) + " must be a constant (an initializer)");
  if (t->dtype == FLOAT) fail(op, std::string(what) + " must be an integer tensor");
  return t->i;
}

// out[n][k] = x[n][idx[k]] for a float or integer payload
Tensor take_columns(const Tensor& x, int64_t N, int64_t C, const std::vector<int64_t>& idx, std::vector<int64_t> dims) {
  Tensor out;
  out.dtype = x.dtype;
  out.elem = x.elem;
  out.dims = std::move(dims);
  const int64_t K = int64_t(idx.size());
  if (x.dtype == FLOAT) {
    out.f.resize(size_t(N * K));
    for (int64_t r = 0; r < N; ++r)
      for (int64_t k = 0; k < K; ++k) out.f[r * K + k] = x.f[r * C + idx[k]];
  } else {
    out.i.resize(size_t(N * K));
    for (int64_t r = 0; r < N; ++r)
      for (int64_t k = 0; k < K; ++k) out.i[r * K + k] = x.i[r * C + idx[k]];
  }
  return out;
}

}  // namespace

int64_t float_to_int64(float v) {
  // 2^63 is the first float past the range; the comparison is false for NaN
  if (!(v >= -9223372036854775808.f && v < 9223372036854775808.f)) return std::numeric_limits<int64_t>::min();
  return int64_t(v);
}

Tensor imputer(const Node& n, const Tensor& x) {
  const char* op = "Imputer";
  if (n.attr("imputed_value_int64s") || n.attr("replaced_value_int64"))
    fail(op, "the int64 attributes (imputed_value_int64s / replaced_value_int64) are not supported");
  float_in(op, x);
  int64_t N, C;
  rows_cols(op, x, N, C);
  const auto* a = n.attr("imputed_value_floats");
  if (!a || (a->floats.size() != 1 && int64_t(a->floats.size()) != C))
    fail(op, "imputed_value_floats must hold 1 or C values");
  const auto& v = a->floats;
  const float rep = n.getf("replaced_value_float", 0.f);
  const bool rep_nan = std::isnan(rep);
  Tensor out = x;
  for (int64_t e = 0; e < N * C; ++e) {
    const float xe = x.f[e];
    const bool hit = rep_nan ? std::isnan(xe) : xe == rep;
    if (hit) out.f[e] = v[v.size() == 1 ? 0 : e % C];
  }
  return out;
}

Tensor array_feature_extractor(const Node& n, const Tensor& x, const Tensor* y, bool y_const) {
  const char* op = "ArrayFeatureExtractor";
  (void)n;
  const auto& idx = int_const(op, "Y (the indices)", y, y_const);
  int64_t N, C;
  rows_cols(op, x, N, C);
  for (int64_t j : idx)
    if (j < 0 || j >= C) fail(op, "index " + std::to_string(j) + " outside [0, " + std::to_string(C) + ")");
  std::vector<int64_t> dims = x.dims.size() == 1 ? std::vector<int64_t>{1, 0} : x.dims;
  dims.back() = int64_t(idx.size());
  return take_columns(x, N, C, idx, dims);
}

Tensor gather(const Node& n, const Tensor& x, const Tensor* idx_t, bool idx_const) {
  const char* op = "Gather";
  const auto& raw = int_const(op, "indices", idx_t, idx_const);
  const int64_t axis = n.geti("axis", 0);
  if (x.dims.size() == 3 && (axis == 2 || axis == -1)) {
    // the last axis of a rank-3 value (a sequence model's [N][C][T]): 1-D indices give [N][C][k], a scalar [N][C]
    if (idx_t->dims.size() > 1) fail(op, "indices must be a scalar or 1-D");
    int64_t R, C;
    rows_cols(op, x, R, C);
    std::vector<int64_t> idx = raw;
    for (auto& j : idx) {
      if (j < -C || j >= C) fail(op, "index " + std::to_string(j) + " outside [-" + std::to_string(C) + ", " + std::to_string(C) + ")");
      if (j < 0) j += C;
    }
    if (idx_t->dims.empty()) {
      if (idx.size() != 1) fail(op, "a scalar index tensor must hold one value");
      return take_columns(x, R, C, idx, {x.dims[0], x.dims[1]});
    }
    return take_columns(x, R, C, idx, {x.dims[0], x.dims[1], int64_t(idx.size())});
  }
  if (x.dims.size() != 2 || (axis != 1 && axis != -1))
    fail(op, "only axis 1 / -1 of a 2-D value is supported (axis " + std::to_string(axis) + ", rank " +
                 std::to_string(x.dims.size()) + ")");
  if (idx_t->dims.size() > 1) fail(op, "indices must be a scalar or 1-D");
  const int64_t N = x.dims[0], C = x.dims[1];
  std::vector<int64_t> idx = raw;
  for (auto& j : idx) {
    if (j < -C || j >= C) fail(op, "index " + std::to_string(j) + " outside [-" + std::to_string(C) + ", " + std::to_string(C) + ")");
    if (j < 0) j += C;
  }
  if (idx_t->dims.empty()) {
    if (idx.size() != 1) fail(op, "a scalar index tensor must hold one value");
    return take_columns(x, N, C, idx, {N});
  }
  return take_columns(x, N, C, idx, {N, int64_t(idx.size())});
}

Tensor slice(const Node& n, const Tensor& x, const Tensor* starts_t, const Tensor* ends_t, const Tensor* axes_t,
             const Tensor* steps_t, bool all_const) {
  const char* op = "Slice";
  if (n.attr("starts") || n.attr("ends") || n.attr("axes"))
    fail(op, "the attribute form (opset < 10) is not supported: starts / ends / axes / steps are inputs");
  const auto& starts = int_const(op, "starts", starts_t, all_const);
  const auto& ends = int_const(op, "ends", ends_t, all_const);
  const size_t k = starts.size();
  if (ends.size() != k) fail(op, "starts and ends differ in length");
  std::vector<int64_t> axes(k), steps(k, 1);
  for (size_t e = 0; e < k; ++e) axes[e] = int64_t(e);
  if (axes_t) axes = int_const(op, "axes", axes_t, all_const);
  if (steps_t) steps = int_const(op, "steps", steps_t, all_const);
  if (axes.size() != k || steps.size() != k) fail(op, "axes / steps must be as long as starts");
  const int64_t rank = int64_t(x.dims.size());
  if (rank < 1) fail(op, "the input must have a feature axis (rank >= 1)");
  int64_t N, C;
  rows_cols(op, x, N, C);
  std::vector<int64_t> idx;
  bool cut = false;
  for (size_t e = 0; e < k; ++e) {
    int64_t ax = axes[e] < 0 ? axes[e] + rank : axes[e];
    if (ax < 0 || ax >= rank) fail(op, "axis " + std::to_string(axes[e]) + " out of range");
    const int64_t dim = x.dims[ax], step = steps[e];
    if (step == 0) fail(op, "a step of 0");
    int64_t s = starts[e], t = ends[e];
    if (s < 0) s += dim;
    if (t < 0) t += dim;
    if (step > 0) {
      s = std::min(std::max<int64_t>(s, 0), dim);
      t = std::min(std::max<int64_t>(t, 0), dim);
    } else {
      s = std::min(std::max<int64_t>(s, 0), dim - 1);
      t = std::min(std::max<int64_t>(t, -1), dim - 1);
    }
    if (ax != rank - 1) {
      if (step != 1 || s != 0 || t != dim) fail(op, "only the last axis may be cut (axis " + std::to_string(ax) + " must keep its full range)");
      continue;
    }
    if (cut) fail(op, "the last axis is named twice");
    cut = true;
    if (step > 0) for (int64_t j = s; j < t; j += step) idx.push_back(j);
    else for (int64_t j = s; j > t; j += step) idx.push_back(j);
  }
  if (!cut) return x;
  std::vector<int64_t> dims = x.dims;
  dims.back() = int64_t(idx.size());
  return take_columns(x, N, C, idx, dims);
}

Tensor one_hot_encoder(const Node& n, const Tensor& x) {
  const char* op = "OneHotEncoder";
  if (n.attr("cats_strings")) fail(op, "cats_strings (string categories) is not supported");
  const auto* a = n.attr("cats_int64s");
  if (!a || a->ints.empty()) fail(op, "cats_int64s is required");
  const auto& cats = a->ints;
  const int64_t K = int64_t(cats.size());
  const bool zeros = n.geti("zeros", 1) != 0;
  const int64_t total = x.numel();
  Tensor out;
  out.dtype = FLOAT;
  out.dims = x.dims;
  out.dims.push_back(K);
  out.f.assign(size_t(total * K), 0.f);
  const bool is_float = x.dtype == FLOAT;
  for (int64_t e = 0; e < total; ++e) {
    bool valid = true;
    int64_t v;
    if (is_float) {
      const float xe = x.f[e];
      valid = std::isfinite(xe) && std::fabs(xe) < 9223372036854775808.f;
      v = valid ? int64_t(std::trunc(xe)) : 0;
    } else {
      v = x.i[e];
    }
    bool matched = false;
    if (valid)
      for (int64_t c = 0; c < K; ++c)
        if (cats[c] == v) {
          out.f[e * K + c] = 1.f;
          matched = true;
        }
    if (!matched && !zeros) fail(op, "zeros = 0 and element " + std::to_string(e) + " matches no category");
  }
  return out;
}

Tensor binarizer(const Node& n, const Tensor& x) {
  float_in("Binarizer", x);
  const float thr = n.getf("threshold", 0.f);
  Tensor out = x;
  for (auto& v : out.f) v = v > thr ? 1.f : 0.f;
  return out;
}

Tensor feature_vectorizer(const Node& n, const std::vector<const Tensor*>& xs) {
  const char* op = "FeatureVectorizer";
  if (xs.empty()) fail(op, "needs at least one input");
  const auto* a = n.attr("inputdimensions");
  if (a && a->ints.size() != xs.size()) fail(op, "inputdimensions must hold one width per input");
  int64_t N = -1, total = 0;
  std::vector<int64_t> widths;
  for (size_t k = 0; k < xs.size(); ++k) {
    const Tensor& t = *xs[k];
    if (t.dims.empty() || t.dims.size() > 2) fail(op, "inputs must be [N] or [N][C]");
    const int64_t w = t.dims.size() == 1 ? 1 : t.dims[1];
    if (N >= 0 && t.dims[0] != N) fail(op, "inputs differ in their row count");
    N = t.dims[0];
    if (a && a->ints[k] != w) fail(op, "inputdimensions[" + std::to_string(k) + "] = " + std::to_string(a->ints[k]) + ", the input has " + std::to_string(w) + " columns");
    widths.push_back(w);
    total += w;
  }
  Tensor out;
  out.dtype = FLOAT;
  out.dims = {N, total};
  out.f.assign(size_t(N * total), 0.f);
  int64_t off = 0;
  for (size_t k = 0; k < xs.size(); ++k) {
    const Tensor& t = *xs[k];
    const int64_t w = widths[k];
    for (int64_t r = 0; r < N; ++r)
      for (int64_t c = 0; c < w; ++c)
        out.f[r * total + off + c] = t.dtype == FLOAT ? t.f[r * w + c] : float(t.i[r * w + c]);
    off += w;
  }
  return out;
}

}  // namespace igp::cols
