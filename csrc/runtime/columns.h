// Column operators of scikit-learn ColumnTransformer front ends (ai.onnx.ml Imputer,
// ArrayFeatureExtractor, OneHotEncoder, Binarizer, FeatureVectorizer; ai.onnx Gather and Slice along
// the feature axis): evaluated by the CPU executor, lowered by the device plan compiler
// (models/plan.py ColumnStep) to one launch of csrc/kernels/columns.hip.
//
// Values are float tensors [N][C] unless said otherwise; N may be 0. Every function throws
// std::runtime_error, with the operator's name in the message, on a malformed node.
#pragma once
#include <cstdint>
#include <vector>

#include "onnx_model.h"

namespace igp::cols {

using onnx::Node;
using onnx::Tensor;

// float -> int64 as Cast defines it here: truncation towards zero; NaN and values outside
// [-2^63, 2^63) give INT64_MIN (what the x86 conversion yields, now spelled out).
int64_t float_to_int64(float v);

// y = hit ? imputed[c] : x; hit = isnan(x) when replaced_value_float is NaN, else x == replaced
// (so -0.0 hits 0.0). imputed_value_floats holds 1 or C values; the *_int64* attributes are refused.
Tensor imputer(const Node& n, const Tensor& x);

// X[:, Y]: Y an int64 constant (flattened), every index in [0, C). Output [N][len(Y)].
Tensor array_feature_extractor(const Node& n, const Tensor& x, const Tensor* y, bool y_const);

// Gather along axis 1 / -1 of a 2-D value with constant int32 / int64 indices: 1-D indices give
// [N][k], a scalar [N]. Negative indices wrap. The last axis (2 / -1) of a rank-3 value [N][C][T] is
// gathered the same way: [N][C][k], a scalar [N][C].
Tensor gather(const Node& n, const Tensor& x, const Tensor* idx, bool idx_const);

// Slice, opset >= 10 form (starts, ends, axes, steps as constants; any non-zero step; ONNX clamping).
// Only the last axis may be cut: an entry for another axis must cover its full range.
Tensor slice(const Node& n, const Tensor& x, const Tensor* starts, const Tensor* ends, const Tensor* axes,
             const Tensor* steps, bool all_const);

// Float or int64 input of any rank -> input shape + [n_cats], f32. A float element matches category
// c when it is finite, |x| < 2^63 and (int64)trunc(x) == c. zeros = 0: an unmatched element throws.
Tensor one_hot_encoder(const Node& n, const Tensor& x);

// y = x > threshold ? 1 : 0 (NaN gives 0)
Tensor binarizer(const Node& n, const Tensor& x);

// Concatenation of the inputs along axis 1; a rank-1 input [N] counts as one column; inputdimensions
// is checked against the widths.
Tensor feature_vectorizer(const Node& n, const std::vector<const Tensor*>& xs);

}  // namespace igp::cols
