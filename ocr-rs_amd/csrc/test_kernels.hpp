// Kernels that were measured, found no faster than what ships and withdrawn from the product: conv_x3w.hip and winograd43_x3.hip are
// linked into libocr_amd_test.so only and reached through its ocr_test_* hooks (test_hooks.hip).  Nothing of libocr_amd.so includes this.
#pragma once
#include "common.hpp"

namespace ocr {

// conv_x3w.hip: the split-bf16 convs with NHWC stores and Cout a multiple of 128 as 256 x 128 tiles on one persistent workgroup per CU
// (bit-identical to conv_igemm's 128-wide split-bf16 tiles); `cus` = CUs of the device
bool conv_x3_wide_applicable(const ConvDesc& d);
void launch_conv_x3_wide(const ConvDesc& d, int cus, hipStream_t s);
// winograd43_x3.hip: the fused F(4x4,3x3) conv of winograd43_fused.hip with its GEMMs on the bf16 matrix cores, f32 operands as three
// bf16 terms each: two pixel blocks per workgroup, one workgroup per CU.  ufrag: winograd43_x3_fragments(winograd_weights(.., 4)).
std::vector<uint16_t> winograd43_x3_fragments(const std::vector<float>& u, int cout, int cin);
void launch_winograd43_x3(const float* x, const void* ufrag, const float* scale, const float* bias, const float* residual,
                          int relu, float* y, int N, int H, int W, int C, int K, int num_cus, hipStream_t s);
#ifdef W43_STAMPS
void winograd43_x3_read_stamps(long long* out);
#endif

}  // namespace ocr
