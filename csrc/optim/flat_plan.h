// The segmented per-tensor plan fused_lars.hip and fused_lamb.hip share: every
// parameter's slot in a flat buffer (padded to 8 elements with zeros) is cut on
// the host, once per layout, into work items of at most kChunkVec vectors:
//   items   int32 [I, 3]  first vector, vector count (<= kChunkVec), tensor
//   tensors int32 [T, 3]  first item, item count, adapted (1) / excluded (0)
//   coef    fp32  [T, 4]  trust ratio, weight decay, |w|, a second norm
// One 256-lane block works on one item, one wave folds one tensor's partials.
// The kernels check each plan entry against the buffers' sizes and skip what
// does not fit, so a damaged plan cannot make them touch memory outside.
#pragma once

#include "flat_step.h"

namespace dmp {

constexpr int kVecPerLane = 4;                      // most vectors of one item a lane owns
constexpr int kChunkVec = kThreads * kVecPerLane;   // 1024 vectors = 8192 elements per work item
constexpr int kItemCols = 3, kTensorCols = 3, kCoefCols = 4;
constexpr int kTrust = 0, kDecay = 1, kWNorm = 2, kGNorm = 3;  // coef[] columns

// The block's work item, or a count of 0 when the entry does not fit the flat.
struct Item {
  int first, count, tensor;
};
__device__ __forceinline__ Item load_item(const int32_t* __restrict__ items, int64_t nvec, int ntensors) {
  const int32_t* it = items + (int64_t)blockIdx.x * kItemCols;
  Item r{it[0], it[1], it[2]};
  const bool ok = r.first >= 0 && r.count >= 0 && r.count <= kChunkVec && (int64_t)r.first + r.count <= nvec &&
                  r.tensor >= 0 && r.tensor < ntensors;
  if (!ok) r.count = 0;
  return r;
}

inline void check_plan(const at::Tensor& t, const char* name, at::ScalarType dtype, int64_t cols, int dev) {
  check_flat(t, name);
  TORCH_CHECK(t.scalar_type() == dtype && t.dim() == 2 && t.size(1) == cols && t.size(0) <= INT32_MAX &&
                  t.get_device() == dev,
              name, " must be a ", dtype, " [n, ", cols, "] tensor on the parameters' device");
}

}  // namespace dmp
