// LAMB (You et al. 2020): AdamW's update direction rescaled per tensor by
// |w| / |update|, over the same FLAT buffers and the same segmented plan
// (flat_plan.h) fused_lars.hip works on.  This is timm's Lamb with
// always_adapt=False and trust_clip=False, after global-norm clipping.  The
// clip and the step count are fused_adamw.hip's (flat_sumsq_partials,
// adamw_prepare: `hyper` = {1 - b1^t, 1 - b2^t, gradient norm, clip
// coefficient} on the device); three kernels per dtype group follow them:
//   lamb_moments    one block per work item: g' = clip g, m = b1 m + (1 - b1) g',
//                   v = b2 v + (1 - b2) g'^2 stored; the direction
//                   u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd_t w
//                   formed in registers; partials[item] = {sum w^2, sum u^2}
//                   (fp32, fixed order, no atomics)
//   lamb_trust      one wave per tensor: folds the tensor's partials in double,
//                   writes coef[t] = {trust, wd_t, |w|, |u|}
//   lamb_flat_step  one block per work item: u again from the stored m, v and
//                   w, w = w - lr trust u, bf16 working copy and the weight EMA
//                   written in the same pass
// u is recomputed, not stored: a stored u would move the same 40 bytes per
// element (+4 written in pass 1, 8 read in pass 3 instead of 12) and cost a
// fourth fp32 flat per parameter; recomputing keeps LAMB's state AdamW's.
// Both passes form u with lamb_direction() from equal fp32 inputs (the m and v
// pass 1 stores are the values it used, w is untouched in between), so the u
// that is applied has the bits of the u whose norm was taken.
//
// Traffic, bf16 gradients and parameters with an fp32 master, per element:
// pass 1 reads g(2) w(4) m(4) v(4) and writes m(4) v(4) = 22 B; pass 3 reads
// m(4) v(4) w(4) and writes w(4) p(2) = 18 B; adamw_flat_step moves 28 B.
//
// Per tensor: trust = |w| / |u|, 1 where |w| or |u| is exactly 0; a non-finite
// norm goes through the formula.  An excluded tensor (tensors[t][2] == 0) has
// wd_t = 0 and trust = 1: plain Adam.  Slot padding is zero in g, m, v and w,
// so u is 0 there (eps > 0) and the padding stays zero in every buffer.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "../api.h"
#include "../common.h"
#include "flat_plan.h"
#include "flat_step.h"

namespace dmp {
namespace {

// hyper[] slots written by adamw_prepare (fused_adamw.hip)
constexpr int kBc1 = 0, kBc2 = 1, kClip = 3, kHyper = 4;
constexpr int kInFlight = 2;  // lamb_moments: vectors a lane holds at once (4 operand sets x 8 x 2 = 64 VGPRs)
static_assert(kVecPerLane % kInFlight == 0, "an item is walked in groups of kInFlight vectors per lane");

// The per-step scalars of the direction, uniform over the grid.
struct Direction {
  float inv_bc1, rsqrt_bc2, eps;
};
__device__ __forceinline__ Direction load_direction(const float* __restrict__ hyper, float eps) {
  return {1.f / hyper[kBc1], 1.f / sqrtf(hyper[kBc2]), eps};
}

// u of one element.  The ONE place it is formed: lamb_moments takes its norm,
// lamb_flat_step applies it, and both must get the same bits.
__device__ __forceinline__ float lamb_direction(float m, float v, float w, float wd, const Direction& d) {
  // sqrt(v) + eps, not m * rsqrt(v): an exactly-zero gradient history must give 0 / eps = 0
  const float denom = fmaf(sqrtf(v), d.rsqrt_bc2, d.eps);
  return fmaf(wd, w, (m * d.inv_bc1) / denom);
}

// Block b walks its item two vectors per lane at a time: moments updated and
// stored, u formed, w^2 and u^2 added per lane in element order; then the wave
// and the block fold in a fixed order.  partials[b] is written on every call,
// {0, 0} for an entry that does not fit.
template <typename G>
__global__ __launch_bounds__(kThreads) void lamb_moments_kernel(
    const float* __restrict__ weight, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
    const G* __restrict__ grad, const int32_t* __restrict__ items, const int32_t* __restrict__ tensors,
    const float* __restrict__ hyper, float* __restrict__ partials, int64_t nvec, int ntensors, float beta1,
    float beta2, float omb1, float omb2, float eps, float weight_decay) {
  __shared__ float red[2][kThreads / kWave];
  const Item it = load_item(items, nvec, ntensors);
  float sw = 0.f, su = 0.f;
  if (it.count != 0) {  // block-uniform
    const float wd = tensors[(int64_t)it.tensor * kTensorCols + 2] != 0 ? weight_decay : 0.f;
    const float clip = hyper[kClip];
    const Direction d = load_direction(hyper, eps);
    for (int base = 0; base < it.count; base += kInFlight * kThreads) {
      float g[kInFlight][8], w[kInFlight][8], m[kInFlight][8], v[kInFlight][8];
#pragma unroll
      for (int k = 0; k < kInFlight; ++k) {
        const int i = base + k * kThreads + threadIdx.x;
        if (i < it.count) {
          const int64_t o = ((int64_t)it.first + i) * 8;
          load8(grad + o, g[k]);
          load8(weight + o, w[k]);
          load8(exp_avg + o, m[k]);
          load8(exp_avg_sq + o, v[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < kInFlight; ++k) {
        const int i = base + k * kThreads + threadIdx.x;
        if (i < it.count) {
          const int64_t o = ((int64_t)it.first + i) * 8;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float gj = g[k][j] * clip;
            m[k][j] = fmaf(beta1, m[k][j], omb1 * gj);
            v[k][j] = fmaf(beta2, v[k][j], omb2 * gj * gj);
            const float u = lamb_direction(m[k][j], v[k][j], w[k][j], wd, d);
            sw = fmaf(w[k][j], w[k][j], sw);
            su = fmaf(u, u, su);
          }
          store8(exp_avg + o, m[k]);
          store8(exp_avg_sq + o, v[k]);
        }
      }
    }
  }
  sw = wave_sum(sw);
  su = wave_sum(su);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red[0][threadIdx.x / kWave] = sw;
    red[1][threadIdx.x / kWave] = su;
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
__global__ __launch_bounds__(kThreads) void lamb_trust_kernel(const float* __restrict__ partials,
                                                              const int32_t* __restrict__ tensors,
                                                              float* __restrict__ coef, int ntensors,
                                                              int64_t nitems, double wd) {
  const int lane = threadIdx.x & (kWave - 1);
  const int t = blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave;
  if (t >= ntensors) return;  // whole waves leave; no barrier follows
  const int32_t* tt = tensors + (int64_t)t * kTensorCols;
  const int begin = tt[0];
  int count = tt[1];
  const bool adapted = tt[2] != 0;
  if (begin < 0 || count < 0 || (int64_t)begin + count > nitems) count = 0;
  double sw = 0.0, su = 0.0;
  for (int i = lane; i < count; i += kWave) {
    const float* p = partials + ((int64_t)begin + i) * 2;
    sw += (double)p[0];
    su += (double)p[1];
  }
  sw = wave_sum(sw);
  su = wave_sum(su);
  if (lane != 0) return;
  const double wn = sqrt(sw), un = sqrt(su);
  double trust = 1.0, decay = 0.0;
  if (adapted) {
    decay = wd;
    // a non-finite norm goes through the formula; only exact zeros are special
    if (sw != 0.0 && su != 0.0) trust = wn / un;
  }
  float* c = coef + (int64_t)t * kCoefCols;
  c[kTrust] = (float)trust;
  c[kDecay] = (float)decay;
  c[kWNorm] = (float)wn;
  c[kGNorm] = (float)un;
}

// Block b updates its item with its tensor's {trust, wd_t}: two uniform loads,
// then 8 elements per lane; moments and weights in, weights and parameter out.
template <typename P, bool MASTER, bool EMA>
__global__ __launch_bounds__(kThreads) void lamb_flat_kernel(
    float* __restrict__ master, const float* __restrict__ exp_avg, const float* __restrict__ exp_avg_sq,
    P* __restrict__ param, const int32_t* __restrict__ items, const float* __restrict__ coef,
    const float* __restrict__ hyper, int64_t nvec, int ntensors, float lr, float eps, float* __restrict__ ema,
    float omd) {
  const Item it = load_item(items, nvec, ntensors);
  if (it.count == 0) return;
  const float step = -lr * coef[(int64_t)it.tensor * kCoefCols + kTrust];
  const float wd = coef[(int64_t)it.tensor * kCoefCols + kDecay];
  const Direction d = load_direction(hyper, eps);
  for (int i = threadIdx.x; i < it.count; i += kThreads) {
    const int64_t o = ((int64_t)it.first + i) * 8;
    float m[8], v[8], w[8];
    load8(exp_avg + o, m);
    load8(exp_avg_sq + o, v);
    load_weights<MASTER>(master, param, o, w);
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = fmaf(step, lamb_direction(m[j], v[j], w[j], wd, d), w[j]);
    store_weights<MASTER>(master, param, o, w);
    ema_update<EMA>(ema, o, w, omd);
  }
}

// What the two streaming passes check beyond flat_step_args.
void check_lamb(const FlatStep& fs, const at::Tensor& items, const at::Tensor& hyper, double eps) {
  TORCH_CHECK(fs.n / 8 <= INT32_MAX, "flat buffer too large for a 32-bit vector index");
  check_plan(items, "items", at::kInt, kItemCols, fs.dev);
  check_flat(hyper, "hyper");
  TORCH_CHECK(hyper.scalar_type() == at::kFloat && hyper.numel() == kHyper && hyper.get_device() == fs.dev,
              "hyper must be fp32 [4] on the parameters' device");
  TORCH_CHECK(eps > 0.0, "eps must be positive (the zero padding of a slot gives u = 0 / eps), got ", eps);
}

}  // namespace

// master / grad / param: as lars_norm_partials; exp_avg / exp_avg_sq: fp32 flat
// moments, updated here; items: int32 [I, 3]; tensors: int32 [T, 3]; hyper: as
// written by adamw_prepare; partials: fp32 [I, 2] = {sum w^2, sum u^2}.
void lamb_moments(const c10::optional<at::Tensor>& master, at::Tensor& exp_avg, at::Tensor& exp_avg_sq,
                  const at::Tensor& grad, const at::Tensor& param, const at::Tensor& items,
                  const at::Tensor& tensors, const at::Tensor& hyper, at::Tensor& partials, double beta1,
                  double beta2, double eps, double weight_decay) {
  const FlatStep fs = flat_step_args(master, grad, param, c10::nullopt, 0.0);
  float* m1 = check_flat_state(exp_avg, "exp_avg", fs);
  float* m2 = check_flat_state(exp_avg_sq, "exp_avg_sq", fs);
  check_lamb(fs, items, hyper, eps);
  check_plan(tensors, "tensors", at::kInt, kTensorCols, fs.dev);
  check_plan(partials, "partials", at::kFloat, 2, fs.dev);
  const int64_t nitems = items.size(0);
  TORCH_CHECK(partials.size(0) == nitems, "partials must have one row per work item");
  if (nitems == 0) return;
  // formed in double, rounded once: what torch's python-float hyper-parameters give
  const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto g) {
    using G = decltype(g);
    hipLaunchKernelGGL((lamb_moments_kernel<G>), dim3((unsigned)nitems), dim3(kThreads), 0, stream, fs.weights(),
                       m1, m2, static_cast<const G*>(fs.grad), items.data_ptr<int32_t>(),
                       tensors.data_ptr<int32_t>(), hyper.data_ptr<float>(), partials.data_ptr<float>(), fs.n / 8,
                       (int)tensors.size(0), (float)beta1, (float)beta2, omb1, omb2, (float)eps,
                       (float)weight_decay);
  };
  if (fs.grad_bf16) launch(__bf16{});
  else launch(float{});
}

// partials: fp32 [I, 2] of lamb_moments; tensors: int32 [T, 3];
// coef: fp32 [T, 4] = {trust ratio, weight decay, |w|, |u|}.
void lamb_trust(const at::Tensor& partials, const at::Tensor& tensors, at::Tensor& coef, double weight_decay) {
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
  hipLaunchKernelGGL(lamb_trust_kernel, dim3((unsigned)((nt + per_block - 1) / per_block)), dim3(kThreads), 0,
                     stream, partials.data_ptr<float>(), tensors.data_ptr<int32_t>(), coef.data_ptr<float>(),
                     (int)nt, partials.size(0), weight_decay);
}

// master / param / ema: as lars_flat_step; exp_avg / exp_avg_sq: the moments
// lamb_moments stored; coef: of lamb_trust; hyper / eps: what lamb_moments got.
// The pass reads no gradient.
void lamb_flat_step(const c10::optional<at::Tensor>& master, const at::Tensor& exp_avg,
                    const at::Tensor& exp_avg_sq, at::Tensor& param, const at::Tensor& items,
                    const at::Tensor& coef, const at::Tensor& hyper, double lr, double eps,
                    const c10::optional<at::Tensor>& ema, double ema_decay) {
  // no gradient here: the parameters stand in for it in the size checks
  const FlatStep fs = flat_step_args(master, param, param, ema, ema_decay);
  const float* m1 = check_flat_state(exp_avg, "exp_avg", fs);
  const float* m2 = check_flat_state(exp_avg_sq, "exp_avg_sq", fs);
  check_lamb(fs, items, hyper, eps);
  check_plan(coef, "coef", at::kFloat, kCoefCols, fs.dev);
  const int64_t nitems = items.size(0);
  if (nitems == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  dispatch_flat_step(fs, [&](auto, auto p, auto m, auto e) {
    using P = decltype(p);
    hipLaunchKernelGGL((lamb_flat_kernel<P, decltype(m)::value, decltype(e)::value>), dim3((unsigned)nitems),
                       dim3(kThreads), 0, stream, fs.master, m1, m2, static_cast<P*>(fs.param),
                       items.data_ptr<int32_t>(), coef.data_ptr<float>(), hyper.data_ptr<float>(), fs.n / 8,
                       (int)coef.size(0), (float)lr, (float)eps, fs.ema, fs.omd);
  });
}

}  // namespace dmp
