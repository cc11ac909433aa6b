// The QuickGELU-epilogue instances of the pointwise contractions (ConvEpi::act == 4, CLIP's MLP): the 128 x 128 kernel of
// conv_gemm.hip for bf16 and for fp32 storage at every operand precision, and the k_gemm_pipe instance, compiled in a
// translation unit of their own so that they build beside the SiLU / GELU instances and leave those as they are.
// conv_gemm.hip's launch_conv_gemm hands such launches here.
#define MDD_CONV_GEMM_QGELU_TU 1
#include "conv_gemm.hip"
