// Launch helpers one .hip source defines and others call (not bound to
// Python).  Declared here only: the defining file includes this header too.
#pragma once

#include <ATen/ATen.h>
#include <c10/util/Optional.h>
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace dmp {

// bn/batchnorm.hip: deterministic fp64 reduce of [2][rb][C] partials into
// [2C+1] moments (the zeroing contract is in common.h)
void bn_reduce_partials_launch(const float* part, int rb, int C, double* sums, double count,
                               hipStream_t stream);
// whether an apply pass over [M, C] bf16 uses non-temporal accesses (set_bn_streaming)
bool bn_streaming(int64_t M, int64_t C);

// conv/gemm_bf16.hip: the split-M partials of a TN GEMM summed into `out`
// (acc: added to it), and the validated accumulation target of a weight
// gradient (undefined tensor: none given)
void split_reduce_launch(const float* pp, int splits, int64_t n, at::Tensor& out, hipStream_t stream,
                         bool acc = false);
at::Tensor acc_target(const c10::optional<at::Tensor>& out, int64_t numel, at::ScalarType dtype,
                      const char* who);

}  // namespace dmp
