// LARS (layer-wise adaptive rate scaling, You et al. 2017) with momentum over
// the same FLAT parameter / gradient buffers fused_sgd.hip works on.  Three
// kernels per dtype group and step, whatever the number of tensors:
//   lars_norm_partials  one block per work item: sum of squares of the
//                       gradient and of the fp32 weights over that item
//                       (fp32, fixed order, no atomics)
//   lars_trust          one wave per tensor: folds the tensor's partials in
//                       double, writes coef[t] = {trust ratio, weight decay,
//                       |w|, |g|}; {1, 0, ..} for a tensor LARS does not adapt
//   lars_flat_step      one block per work item: d = trust * (g + wd * w),
//                       m = mu * m + d, w -= lr * m, bf16 working copy written
//                       in the same pass
// Norms and trust ratios never leave the device, so step() has no host sync and
// a step captured into a hipGraph stays correct on replay.  lr is a host
// scalar outside the momentum, as in the SGD kernel.
//
// Every parameter's slot in a flat buffer is padded to 8 elements with zeros
// (ddp/reducer.cpp kAlignElems, the list layout of ops/optim.py), so an
// 8-element vector belongs to one tensor and a slot's sum of squares is its
// tensor's.  The host cuts every slot into work items of at most kChunkVec
// vectors, once per layout (the "plan"):
//   items   int32 [I, 3]  first vector, vector count (<= kChunkVec), tensor
//   tensors int32 [T, 3]  first item, item count, adapted (1) / excluded (0)
// The kernels check each plan entry against the buffers' sizes and skip what
// does not fit, so a damaged plan cannot make them touch memory outside.
//
// Semantics (adapted tensor): trust = eta * |w| / (|g| + wd * |w| + eps), 1
// where |w| or |g| is exactly 0; excluded tensor: trust = 1 and no decay.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "../api.h"
#include "../common.h"
#include "flat_step.h"

namespace dmp {
namespace {

constexpr int kVecPerLane = 4;                      // norm kernel: vectors in flight per lane
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

// Block b reduces its item: partials[b] = {sum g^2, sum w^2}.  Every lane adds
// its (up to) 4 x 8 squares in element order, the wave and the block fold in a
// fixed order; every slot is written on every call.
template <typename G>
__global__ __launch_bounds__(kThreads) void lars_norm_kernel(const G* __restrict__ grad,
                                                             const float* __restrict__ weight,
                                                             const int32_t* __restrict__ items,
                                                             float* __restrict__ partials, int64_t nvec) {
  __shared__ float red[2][kThreads / kWave];
  const Item it = load_item(items, nvec, INT32_MAX);
  float g[kVecPerLane][8], w[kVecPerLane][8];
#pragma unroll
  for (int k = 0; k < kVecPerLane; ++k) {
    const int i = threadIdx.x + k * kThreads;
    if (i < it.count) {
      const int64_t o = ((int64_t)it.first + i) * 8;
      load8(grad + o, g[k]);
      load8(weight + o, w[k]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) g[k][j] = w[k][j] = 0.f;
    }
  }
  float sg = 0.f, sw = 0.f;
#pragma unroll
  for (int k = 0; k < kVecPerLane; ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sg = fmaf(g[k][j], g[k][j], sg);
      sw = fmaf(w[k][j], w[k][j], sw);
    }
  }
  sg = wave_sum(sg);
  sw = wave_sum(sw);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red[0][threadIdx.x / kWave] = sg;
    red[1][threadIdx.x / kWave] = sw;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kThreads / kWave; ++i) s += red[threadIdx.x][i];
    partials[(int64_t)blockIdx.x * 2 + threadIdx.x] = s;
  }
}

// Wave w of block b owns tensor t = 4 b + w: lane l adds the partials of the
// tensor's items l, l + 64, ... in double, the wave folds them (xor butterfly,
// the same order in every lane and on every call), lane 0 writes coef[t].
__global__ __launch_bounds__(kThreads) void lars_trust_kernel(const float* __restrict__ partials,
                                                              const int32_t* __restrict__ tensors,
                                                              float* __restrict__ coef, int ntensors,
                                                              int64_t nitems, double eta, double wd,
                                                              double eps) {
  const int lane = threadIdx.x & (kWave - 1);
  const int t = blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave;
  if (t >= ntensors) return;  // whole waves leave; no barrier follows
  const int32_t* tt = tensors + (int64_t)t * kTensorCols;
  const int begin = tt[0];
  int count = tt[1];
  const bool adapted = tt[2] != 0;
  if (begin < 0 || count < 0 || (int64_t)begin + count > nitems) count = 0;
  double sg = 0.0, sw = 0.0;
  for (int i = lane; i < count; i += kWave) {
    const float* p = partials + ((int64_t)begin + i) * 2;
    sg += (double)p[0];
    sw += (double)p[1];
  }
  sg = wave_sum(sg);
  sw = wave_sum(sw);
  if (lane != 0) return;
  const double gn = sqrt(sg), wn = sqrt(sw);
  double trust = 1.0, decay = 0.0;
  if (adapted) {
    decay = wd;
    // a non-finite norm goes through the formula; only exact zeros are special
    if (sg != 0.0 && sw != 0.0) trust = eta * wn / (gn + wd * wn + eps);
  }
  float* c = coef + (int64_t)t * kCoefCols;
  c[kTrust] = (float)trust;
  c[kDecay] = (float)decay;
  c[kWNorm] = (float)wn;
  c[kGNorm] = (float)gn;
}

// Block b updates its item with its tensor's {trust, decay}: two uniform
// loads, then the stream of sgd_flat_kernel (8 elements per lane; master,
// momentum and gradient in; master, momentum and parameter out).
template <typename G, typename P, bool MASTER, bool EMA>
__global__ __launch_bounds__(kThreads) void lars_flat_kernel(float* __restrict__ master,
                                                             float* __restrict__ mom,
                                                             const G* __restrict__ grad, P* __restrict__ param,
                                                             const int32_t* __restrict__ items,
                                                             const float* __restrict__ coef, int64_t nvec,
                                                             int ntensors, float lr, float momentum,
                                                             float* __restrict__ ema, float omd) {
  const Item it = load_item(items, nvec, ntensors);
  if (it.count == 0) return;
  const float trust = coef[(int64_t)it.tensor * kCoefCols + kTrust];
  const float wd = coef[(int64_t)it.tensor * kCoefCols + kDecay];
  for (int i = threadIdx.x; i < it.count; i += kThreads) {
    const int64_t o = ((int64_t)it.first + i) * 8;
    float g[8], w[8], m[8];
    load8(grad + o, g);
    load_weights<MASTER>(master, param, o, w);
    load8(mom + o, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = trust * fmaf(wd, w[j], g[j]);
      m[j] = fmaf(momentum, m[j], d);
      w[j] = fmaf(-lr, m[j], w[j]);
    }
    store8(mom + o, m);
    store_weights<MASTER>(master, param, o, w);
    ema_update<EMA>(ema, o, w, omd);
  }
}

void check_plan(const at::Tensor& t, const char* name, at::ScalarType dtype, int64_t cols, int dev) {
  check_flat(t, name);
  TORCH_CHECK(t.scalar_type() == dtype && t.dim() == 2 && t.size(1) == cols && t.size(0) <= INT32_MAX &&
                  t.get_device() == dev,
              name, " must be a ", dtype, " [n, ", cols, "] tensor on the parameters' device");
}

// The common checks, and that a plan's int32 vector indices reach every vector of the flats.
FlatStep lars_args(const c10::optional<at::Tensor>& master, const at::Tensor& grad, const at::Tensor& param,
                   const c10::optional<at::Tensor>& ema = c10::nullopt, double ema_decay = 0.0) {
  const FlatStep fs = flat_step_args(master, grad, param, ema, ema_decay);
  TORCH_CHECK(fs.n / 8 <= INT32_MAX, "flat buffer too large for a 32-bit vector index");
  return fs;
}

}  // namespace

int64_t lars_chunk_elems() { return (int64_t)kChunkVec * 8; }
int64_t lars_fold_threads() { return kWave; }

// grad / param: bf16 or fp32 flats, numel a multiple of 8; master: fp32 flat
// (undefined when `param` is fp32).  items: int32 [I, 3]; partials: fp32 [I, 2].
void lars_norm_partials(const c10::optional<at::Tensor>& master, const at::Tensor& grad,
                        const at::Tensor& param, const at::Tensor& items, at::Tensor& partials) {
  const FlatStep fs = lars_args(master, grad, param);
  check_plan(items, "items", at::kInt, kItemCols, fs.dev);
  check_plan(partials, "partials", at::kFloat, 2, fs.dev);
  const int64_t nitems = items.size(0);
  TORCH_CHECK(partials.size(0) == nitems, "partials must have one row per work item");
  if (nitems == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  if (fs.grad_bf16)
    hipLaunchKernelGGL((lars_norm_kernel<__bf16>), dim3((unsigned)nitems), dim3(kThreads), 0, stream,
                       static_cast<const __bf16*>(fs.grad), fs.weights(), items.data_ptr<int32_t>(),
                       partials.data_ptr<float>(), fs.n / 8);
  else
    hipLaunchKernelGGL((lars_norm_kernel<float>), dim3((unsigned)nitems), dim3(kThreads), 0, stream,
                       static_cast<const float*>(fs.grad), fs.weights(), items.data_ptr<int32_t>(),
                       partials.data_ptr<float>(), fs.n / 8);
}

// partials: fp32 [I, 2] of lars_norm_partials; tensors: int32 [T, 3];
// coef: fp32 [T, 4] = {trust ratio, weight decay, |w|, |g|}.
void lars_trust(const at::Tensor& partials, const at::Tensor& tensors, at::Tensor& coef,
                double trust_coefficient, double weight_decay, double eps) {
  check_flat(partials, "partials");
  const int dev = partials.get_device();
  check_plan(partials, "partials", at::kFloat, 2, dev);
  check_plan(tensors, "tensors", at::kInt, kTensorCols, dev);
  check_plan(coef, "coef", at::kFloat, kCoefCols, dev);
  const int64_t nt = tensors.size(0);
  TORCH_CHECK(coef.size(0) == nt, "coef must have one row per tensor");
  if (nt == 0) return;
  const int per_block = kThreads / kWave;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(lars_trust_kernel, dim3((unsigned)((nt + per_block - 1) / per_block)), dim3(kThreads), 0,
                     stream, partials.data_ptr<float>(), tensors.data_ptr<int32_t>(), coef.data_ptr<float>(),
                     (int)nt, partials.size(0), trust_coefficient, weight_decay, eps);
}

// master: fp32 flat (or undefined when `param` is fp32 and is its own master)
// mom: fp32 flat momentum; grad / param: bf16 or fp32 flats; items / coef: as above.
// ema: fp32 flat average of the fp32 weights, ema += (1 - ema_decay) * (w - ema)
// in the same pass (undefined: none); slot padding no work item covers is not touched.
void lars_flat_step(const c10::optional<at::Tensor>& master, at::Tensor& mom, const at::Tensor& grad,
                    at::Tensor& param, const at::Tensor& items, const at::Tensor& coef, double lr,
                    double momentum, const c10::optional<at::Tensor>& ema, double ema_decay) {
  const FlatStep fs = lars_args(master, grad, param, ema, ema_decay);
  float* mo = check_flat_state(mom, "mom", fs);
  check_plan(items, "items", at::kInt, kItemCols, fs.dev);
  check_plan(coef, "coef", at::kFloat, kCoefCols, fs.dev);
  const int64_t nitems = items.size(0);
  if (nitems == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  dispatch_flat_step(fs, [&](auto g, auto p, auto m, auto e) {
    using G = decltype(g);
    using P = decltype(p);
    hipLaunchKernelGGL((lars_flat_kernel<G, P, decltype(m)::value, decltype(e)::value>), dim3((unsigned)nitems),
                       dim3(kThreads), 0, stream, fs.master, mo, static_cast<const G*>(fs.grad),
                       static_cast<P*>(fs.param), items.data_ptr<int32_t>(), coef.data_ptr<float>(), fs.n / 8,
                       (int)coef.size(0), (float)lr, (float)momentum, fs.ema, fs.omd);
  });
}

}  // namespace dmp
