// The ReLU-epilogue instances of the implicit-GEMM convolution (ConvEpi::act == 3, NF-ResNet): the kernels of
// conv_gemm.hip compiled a second time with ACT = 3 in a translation unit of their own, so that they build beside the
// SiLU / GELU instances instead of after them.  conv_gemm.hip's launch_conv_gemm hands such launches here.
#define MDD_CONV_GEMM_RELU_TU 1
#include "conv_gemm.hip"
