// Operators of temporal-convolution (Conv1D / TCN) sequence models: ai.onnx Conv (1-D), Pad
// (constant), GlobalAveragePool / GlobalMaxPool and ReduceMean / ReduceMax / ReduceSum: evaluated by
// the CPU executor, lowered by the device plan compiler (models/plan.py ConvStep / SeqPoolStep) to
// csrc/kernels/conv1d.hip.
//
// Values are float tensors. Every function throws std::runtime_error, with the operator's name in
// the message, on a malformed node; none reads outside its operands.
#pragma once
#include <cstdint>
#include <vector>

#include "onnx_model.h"

namespace igp::conv {

using onnx::Node;
using onnx::Tensor;

// Conv, 1-D: X [N][C][L], W [M][C][k] (a constant), B [M] optional -> [N][M][L + pads - d (k - 1)].
//   y[n][m][t] = B[m] + sum_c sum_j W[m][c][j] * x[n][c][t - pad_begin + j d]   (zero outside [0, L))
// Attributes kernel_shape, dilations, pads [begin, end], strides, group, auto_pad (NOTSET, VALID,
// SAME_UPPER, SAME_LOWER: the odd step of an odd total goes to the end / to the beginning). group != 1,
// a stride other than 1 and 2-D / 3-D kernels are refused. Each element is accumulated in double, in
// the order c then j, and rounded once.
Tensor conv1d(const Node& n, const Tensor& x, const Tensor& w, bool w_const, const Tensor* b);

// Pad, mode constant, any rank: pads [begin_0 .. begin_r-1, end_0 .. end_r-1] >= 0 and the value as
// constant inputs (opset >= 11) or as the attributes pads / value (opset 2).
Tensor pad(const Node& n, const Tensor& x, const Tensor* pads, const Tensor* value, bool all_const, bool has_axes);

// GlobalAveragePool / GlobalMaxPool: X [N][C][d...] -> [N][C][1...]. The mean is summed in double.
Tensor global_pool(const char* op, const Tensor& x);

// ReduceMean / ReduceMax / ReduceSum over `axes` (the attribute, or a constant input; empty: every
// axis unless noop_with_empty_axes), keepdims 1 (default) or 0. Mean and sum run in double.
// Max here and in GlobalMaxPool: a NaN among the reduced elements makes the result NaN.
Tensor reduce(const Node& n, const Tensor& x, const Tensor* axes, bool axes_const);

}  // namespace igp::conv
