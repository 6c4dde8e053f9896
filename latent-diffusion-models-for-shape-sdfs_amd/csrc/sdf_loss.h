// DeepSDF's clamped-L1 term on the decoder's pre-tanh output, shared by the auto-decoder training
// loss (autodecoder.hip, sdf_l1_kernel) and the frozen-decoder gradient kernel (decoder_grad.hip,
// loss mode): one source, so both differentiate the same function.
#pragma once
#include <math.h>

namespace ldm {

__device__ __forceinline__ float clampd(float x, float d) { return fminf(fmaxf(x, -d), d); }

// Per element: loss term and d/d pre.  Written out (no fast-math intrinsics) so the tanh
// matches the C library's within an ulp or two.
__device__ __forceinline__ float sdf_l1_term(float pre, float gt, float delta, float scale,
                                             float& grad) {
    const float pred = tanhf(pre);
    const float diff = clampd(pred, delta) - clampd(gt, delta);
    const float sg = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
    const bool pass = pred >= -delta && pred <= delta;
    grad = pass ? scale * sg * (1.f - pred * pred) : 0.f;
    return fabsf(diff);
}

}  // namespace ldm
