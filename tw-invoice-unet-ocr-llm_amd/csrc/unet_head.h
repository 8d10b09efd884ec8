// Internal (non-ABI) declarations of the output head's kernels (unet_head.hip), shared with the C-ABI host layer:
// out_conv = Conv2d(64, C, 1) (unet_model.py:50) forward and backward on a stored feature map
// (unet_head_forward / unet_head_backward, include/unet_mi355x.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "../../include/unet_mi355x.h"

namespace unet {

constexpr int kHeadK = 64;        // input channels of out_conv
constexpr int kHeadSpan = 4096;   // pixels of one image that one block of the backward's first launch reduces: a
                                  // compile-time constant, so the summation tree depends on (N, H, W) only
constexpr int kHeadFwdTile = 1024;   // pixels of one image per block of the forward / grad_feat kernels

inline long long head_spans(long long hw) { return (hw + kHeadSpan - 1) / kHeadSpan; }
inline long long head_tiles(long long hw) { return (hw + kHeadFwdTile - 1) / kHeadFwdTile; }
// scratch bytes of a backward over N images of hw pixels with C classes: N * head_spans(hw) slabs of
// 64 C + C fp64 partials
size_t head_scratch_bytes(long long N, long long hw, int C);

// feat / feat_dtype below: the feature map [N][64][H][W] as fp32 (UNET_DTYPE_F32), fp16 (UNET_DTYPE_F16) or bf16
// (UNET_DTYPE_BF16); any other dtype is hipErrorInvalidValue.  A 16-bit feature is widened to fp32 exactly, then the
// fp32 arithmetic runs: the outputs are the bits of the fp32 call on the widened tensor.

// logits[n][c][p] = b[c] + sum_k w[c][k] feat[n][k][p]: one fmaf chain from the bias, k ascending
hipError_t launch_head_forward(const void* feat, int feat_dtype, const float* w, const float* b, float* logits, int N,
                               int C, int H, int W, hipStream_t s);

// grad_w / grad_b (both or neither) through the slabs of `scratch`; grad_feat (or nullptr) element-wise
hipError_t launch_head_backward(const void* feat, int feat_dtype, const float* g, const float* w, float* grad_w,
                                float* grad_b, float* grad_feat, int N, int C, int H, int W, void* scratch,
                                hipStream_t s);

}  // namespace unet
