// bev_act.h -- internal: activation functions shared by the conv / depthwise / BatchNorm kernels.
#pragma once
#include <hip/hip_runtime.h>

// Forward ReLU as IEEE-754-2019 maximum(t, +0), one v_maximum3_f32: a NaN stays a NaN (torch.relu / clamp_min; the
// `t > 0 ? t : 0` and fmaxf spellings return 0 for it), -0 becomes +0 (maximum orders -0 < +0) and every other
// value keeps its bits.  The backward masks (`y > 0 ? g : 0`) are separate code and are not spelled with this.
__device__ __forceinline__ float relu_f(float t) { return __builtin_elementwise_maximum(t, 0.0f); }
// NaN-propagating maximum of two values (torch's max_pool2d): the fused stem max-pool's combine
__device__ __forceinline__ float max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }

// SiLU t * sigmoid(t) on the hardware exp2 / reciprocal (v_exp_f32, v_rcp_f32): a few ulp from torch's
// x / (1 + exp(-x)) (relative error <= ~1e-6 for |t| < 100), at ~5 VALU instead of libm expf + an IEEE division
// (~30): the SiLU epilogues of the EfficientNet trunk are a large share of its memory-bound layers' issue time.
__device__ __forceinline__ float silu_hw(float t) {
    return t * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t * -1.4426950408889634f));
}
__device__ __forceinline__ float sigmoid_hw(float t) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t * -1.4426950408889634f));
}
