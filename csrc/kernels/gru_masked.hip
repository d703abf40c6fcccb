// The MASKED = 1 (ONNX sequence_lens) instances of gru.hip's batch-parallel kernels, in a
// translation unit of their own: they compile beside gru.hip instead of doubling its build time,
// and gru.hip's own instances stay what they were. Defines launch_gru_masked.
#define IGP_GRU_MASKED_TU 1
#include "gru.hip"
