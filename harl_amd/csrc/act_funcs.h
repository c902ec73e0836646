// act_funcs.h -- the activation functions other than ReLU (harl/utils/models_tools.py:28-50: sigmoid, tanh, leaky_relu, selu),
// ONE definition for the element-wise launches of the composed 64 / 128-wide route (elementwise.hip) and for the epilogues of
// k_panel_rect<MT, MODE, ACT> (rect.hip).  ACT ids: 1 leaky_relu, 2 tanh, 3 sigmoid, 4 selu.  The backward takes act' from the
// activation VALUE a (tanh: 1 - a^2, sigmoid: a (1 - a), leaky_relu: a > 0 ? 1 : 0.01, selu: a > 0 ? scale : a + scale alpha).
#pragma once
#include <hip/hip_runtime.h>

namespace harl {
constexpr float SELU_SCALE = 1.0507009873554804934193349852946f, SELU_ALPHA = 1.6732632423543772848170429916717f;

__device__ __forceinline__ float act_value(float z, int act) {
  switch (act) {
    case 1: return z > 0.f ? z : 0.01f * z;
    case 2: return tanhf(z);
    case 3: return 1.0f / (1.0f + expf(-z));
    default: return z > 0.f ? SELU_SCALE * z : (SELU_SCALE * SELU_ALPHA) * (expf(z) - 1.0f);
  }
}
__device__ __forceinline__ float act_slope_from_value(float a, int act) {
  switch (act) {
    case 1: return a > 0.f ? 1.0f : 0.01f;
    case 2: return 1.0f - a * a;
    case 3: return a * (1.0f - a);
    default: return a > 0.f ? SELU_SCALE : a + SELU_SCALE * SELU_ALPHA;
  }
}
}  // namespace harl
