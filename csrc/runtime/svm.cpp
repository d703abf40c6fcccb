#include "svm.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#include "trees.h"

namespace igp::svm {
namespace {

const std::vector<float>& floats(const onnx::Node& n, const char* name) {
  static const std::vector<float> none;
  auto a = n.attr(name);
  return a ? a->floats : none;
}

[[noreturn]] void fail(const onnx::Node& n, const std::string& what) {
  throw std::runtime_error(n.op_type + ": " + what);
}

}  // namespace

SvmModel compile(const onnx::Node& n) {
  SvmModel m;
  m.classifier = n.op_type == "SVMClassifier";
  const std::string kt = n.gets("kernel_type", "LINEAR");
  if (kt == "LINEAR") m.kernel = LINEAR;
  else if (kt == "POLY") m.kernel = POLY;
  else if (kt == "RBF") m.kernel = RBF;
  else if (kt == "SIGMOID") m.kernel = SIGMOID;
  else fail(n, "unknown kernel_type " + kt);
  const auto& kp = floats(n, "kernel_params");
  if (kp.size() < 3) fail(n, "kernel_params must hold gamma, coef0 and degree (" + std::to_string(kp.size()) + " given)");
  m.gamma = kp[0];
  m.coef0 = kp[1];
  m.degree = kp[2];
  if (!std::isfinite(m.gamma) || !std::isfinite(m.coef0) || !std::isfinite(m.degree)) fail(n, "non-finite kernel_params");

  const std::string p = n.gets("post_transform", "NONE");
  if (p == "NONE") m.post = trees::NONE;
  else if (p == "LOGISTIC") m.post = trees::LOGISTIC;
  else if (p == "SOFTMAX") m.post = trees::SOFTMAX;
  else if (p == "SOFTMAX_ZERO") m.post = trees::SOFTMAX_ZERO;
  else if (p == "PROBIT") m.post = trees::PROBIT;
  else fail(n, "unknown post_transform " + p);

  m.sv = floats(n, "support_vectors");
  m.coef = floats(n, "coefficients");
  const auto& rho = floats(n, "rho");
  if (m.classifier) {
    std::vector<int64_t> vpc;
    if (auto a = n.attr("vectors_per_class")) vpc = a->ints;
    size_t n_labels = 0;
    if (auto a = n.attr("classlabels_ints")) { m.classlabels = a->ints; n_labels = a->ints.size(); }
    else if (auto s = n.attr("classlabels_strings")) {
      n_labels = s->strings.size();
      for (size_t k = 0; k < n_labels; ++k) m.classlabels.push_back(int64_t(k));
    }
    if (vpc.size() > 2 || n_labels > 2)
      fail(n, "more than two classes are not supported (" + std::to_string(std::max(vpc.size(), n_labels)) + " given)");
    if (vpc.empty()) fail(n, "the linear-SVC form (empty vectors_per_class) is not supported");
    if (vpc.size() != 2 || n_labels != 2) fail(n, "a two-class model needs two classlabels and two vectors_per_class entries");
    if (vpc[0] < 0 || vpc[1] < 0) fail(n, "negative vectors_per_class");
    m.n_sv = vpc[0] + vpc[1];
    const auto& pa = floats(n, "prob_a");
    const auto& pb = floats(n, "prob_b");
    if (pa.empty() != pb.empty()) fail(n, "prob_a and prob_b must be given together");
    if (!pa.empty()) {
      if (pa.size() != 1 || pb.size() != 1) fail(n, "prob_a / prob_b must hold one value for two classes");
      if (!std::isfinite(pa[0]) || !std::isfinite(pb[0])) fail(n, "non-finite prob_a / prob_b");
      m.platt = true;
      m.prob_a = pa[0];
      m.prob_b = pb[0];
    }
  } else {
    m.n_sv = n.geti("n_supports", 0);
    m.one_class = n.geti("one_class", 0) != 0;
    if (n.attr("prob_a") || n.attr("prob_b")) fail(n, "prob_a / prob_b belong to SVMClassifier");
  }
  if (m.n_sv < 1) fail(n, "no support vectors (the linear form with n_supports = 0 is not supported)");
  if (m.sv.empty() || int64_t(m.sv.size()) % m.n_sv)
    fail(n, "support_vectors holds " + std::to_string(m.sv.size()) + " values, not a multiple of the " +
                std::to_string(m.n_sv) + " vectors");
  m.n_feat = int64_t(m.sv.size()) / m.n_sv;
  if (int64_t(m.coef.size()) != m.n_sv)
    fail(n, std::to_string(m.coef.size()) + " coefficients for " + std::to_string(m.n_sv) + " support vectors");
  if (rho.size() != 1) fail(n, "rho must hold one value (" + std::to_string(rho.size()) + " given)");
  m.rho = rho[0];
  if (!std::isfinite(m.rho)) fail(n, "non-finite rho");
  for (float v : m.sv) if (!std::isfinite(v)) fail(n, "non-finite support vector");
  for (float v : m.coef) if (!std::isfinite(v)) fail(n, "non-finite coefficient");
  return m;
}

void decision(const SvmModel& m, const float* X, int64_t n, int64_t n_feat, float* dec) {
  if (n_feat != m.n_feat)
    throw std::runtime_error("SVM: input width " + std::to_string(n_feat) + " != support vector width " +
                             std::to_string(m.n_feat));
  const int64_t S = m.n_sv, F = m.n_feat;
  const double g = m.gamma, c0 = m.coef0, deg = m.degree;
  for (int64_t r = 0; r < n; ++r) {
    const float* x = X + r * F;
    double acc = 0;
    for (int64_t i = 0; i < S; ++i) {
      const float* s = &m.sv[i * F];
      double d = 0;
      if (m.kernel == RBF) {
        for (int64_t k = 0; k < F; ++k) {
          const double t = double(x[k]) - double(s[k]);
          d += t * t;
        }
      } else {
        for (int64_t k = 0; k < F; ++k) d += double(x[k]) * double(s[k]);
      }
      double kv;
      switch (m.kernel) {
        case POLY: kv = std::pow(g * d + c0, deg); break;
        case RBF: kv = std::exp(-g * d); break;
        case SIGMOID: kv = std::tanh(g * d + c0); break;
        default: kv = d;
      }
      acc += double(m.coef[i]) * kv;
    }
    dec[r] = float(acc + double(m.rho));
  }
}

}  // namespace igp::svm
