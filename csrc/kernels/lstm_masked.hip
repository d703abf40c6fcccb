// The MASKED = 1 (ONNX sequence_lens) instances of lstm_kernel, in a translation unit of their
// own (see gru_masked.hip). Defines launch_lstm_masked.
#define IGP_LSTM_MASKED_TU 1
#include "lstm.hip"
