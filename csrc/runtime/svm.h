// ai.onnx.ml SVMRegressor (SVR, one-class) and the two-class SVC form of SVMClassifier, compiled
// from node attributes into one SvmModel: evaluated by the CPU executor and read by the device
// plan compiler (models/plan.py SVMStep).
//
//   dec(x) = sum_i coef[i] * K(x, sv_i) + rho,   d = x . s
//   LINEAR d | POLY (gamma d + coef0)^degree | RBF exp(-gamma |x - s|^2) | SIGMOID tanh(gamma d + coef0)
//
// Regressor: Y = dec, or with one_class dec > 0 ? 1 : -1; then the post transform. Classifier
// (libsvm's orientation, dec > 0 votes for classlabels[0]): scores [dec, -dec] through the post
// transform; with prob_a / prob_b (Platt) [p0, 1 - p0], p0 = 1 / (1 + exp(prob_a dec + prob_b)),
// which are probabilities already and take no post transform.
#pragma once
#include <cstdint>
#include <vector>

#include "onnx_model.h"

namespace igp::svm {

enum Kernel : int32_t { LINEAR = 0, POLY = 1, RBF = 2, SIGMOID = 3 };

struct SvmModel {
  bool classifier = false;
  int32_t kernel = LINEAR;
  float gamma = 0, coef0 = 0, degree = 0;
  int64_t n_sv = 0, n_feat = 0;
  std::vector<float> sv;    // [S][F]
  std::vector<float> coef;  // [S]
  float rho = 0;
  int32_t post = 0;         // trees::Post code (NONE / LOGISTIC ... as the linear operators)
  bool one_class = false;   // regressor only
  bool platt = false;       // classifier only
  float prob_a = 0, prob_b = 0;
  std::vector<int64_t> classlabels;  // two entries (string labels: 0, 1)
};

// Throws std::runtime_error with a message on a malformed node, more than two classes or the
// linear-SVC form (empty vectors_per_class).
SvmModel compile(const onnx::Node& node);

// dec for n rows of n_feat columns: f32 inputs, double accumulation (direct differences for RBF),
// one rounding at the output.
void decision(const SvmModel& m, const float* X, int64_t n, int64_t n_feat, float* dec);

}  // namespace igp::svm
