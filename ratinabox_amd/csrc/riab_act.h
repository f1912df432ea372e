// utils.activate (reference utils.py:919-1026) on the device: shared by the FeedForwardLayer GEMM (riab_ff.hip) and the
// fused multi-layer perceptron (riab_mlp.hip), so that one layer evaluated by either has the same bits.
#pragma once

#include "riab_device.h"

namespace riab {

// Returns f(x), writes df/dx.  ACT is a template parameter so that the epilogue of a lane is straight-line code.
template <int ACT>
__device__ __forceinline__ float activate(float x, float p0, float p1, float p2, float p3, float* d) {
  if constexpr (ACT == RIAB_ACT_LINEAR) {
    *d = 1.0f;
    return x;
  } else if constexpr (ACT == RIAB_ACT_SIGMOID) {  // p0 max_fr, p1 min_fr, p2 mid_x, p3 beta = ln(19)/(width_x/2)
    const float s = 1.0f / (1.0f + expf(-p3 * (x - p2)));
    const float f = (p0 - p1) * s + p1;
    *d = p3 * (f - p1) * (1.0f - (f - p1) / (p0 - p1));
    return f;
  } else if constexpr (ACT == RIAB_ACT_RELU) {  // p0 gain, p1 threshold
    *d = p0 * ((x - p1) > 0.0f ? 1.0f : 0.0f);
    return p0 * fmaxf(0.0f, x - p1);
  } else if constexpr (ACT == RIAB_ACT_TANH) {  // the reference's derivative ignores the threshold (utils.py:998)
    const float th = tanhf(x);
    *d = p0 * (1.0f - th * th);
    return p0 * tanhf(x - p1);
  } else if constexpr (ACT == RIAB_ACT_RETANH) {
    const float th = tanhf(x);
    *d = p0 * (1.0f - th * th) * ((x - p1) > 0.0f ? 1.0f : 0.0f);
    return p0 * fmaxf(0.0f, tanhf(x - p1));
  } else {  // RIAB_ACT_SOFTMAX: "softmax" in the reference is softplus, gain*log(1+exp(x-thr))
    const float z = x - p1;
    *d = p0 / (1.0f + expf(-z));
    return p0 * (z > 20.0f ? z : log1pf(expf(z)));
  }
}

}  // namespace riab
