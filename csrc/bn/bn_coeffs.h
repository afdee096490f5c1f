// The per-channel coefficients of a training-mode BN forward, shared by every
// kernel that applies one (batchnorm.hip, bn_apply_gram.hip): one definition,
// so their outputs agree bit for bit.
#pragma once

#include "../common.h"

namespace dmp {

// Per-channel forward coefficients from (possibly all-reduced) moments.
__device__ __forceinline__ void fwd_coeffs(const double* __restrict__ sums, int C, int c,
                                           const float* __restrict__ w, const float* __restrict__ b,
                                           float eps, float& mean, float& invstd, float& var_b,
                                           float& scale, float& shift) {
  const double n = sums[2 * C];
  const double m = sums[c] / n;
  double v = sums[C + c] / n - m * m;
  v = v < 0.0 ? 0.0 : v;
  mean = (float)m;
  var_b = (float)v;
  invstd = (float)(1.0 / sqrt(v + (double)eps));
  const float ww = w ? w[c] : 1.f, bb = b ? b[c] : 0.f;
  scale = ww * invstd;
  shift = bb - mean * scale;
}

}  // namespace dmp
