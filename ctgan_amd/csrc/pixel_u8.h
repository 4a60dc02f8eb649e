// pixel_u8.h - the score-sample quantisation shared by ctgan_pixels_u8 (elementwise.hip) and ctgan_score_input (score_cifar.hip).
#pragma once
#include <hip/hip_runtime.h>

// trunc((x + 1) * scale) clamped to [0, 255].  Add then multiply, each rounded on its own (no fused multiply-add), so that finite
// inputs are bit-equal to ((x + 1.) * scale).to(int32).clamp(0, 255); a non-finite input gives 0.
__device__ __forceinline__ unsigned pixel_u8(float x, float scale) {
    const float v = __fmul_rn(__fadd_rn(x, 1.0f), scale);
    if (!isfinite(x) || !(v > 0.f)) return 0u;
    return v >= 256.f ? 255u : (unsigned)(int)v;
}
