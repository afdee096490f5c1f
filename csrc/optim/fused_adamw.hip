// Single-launch AdamW (decoupled weight decay) with global-norm gradient
// clipping over the same FLAT parameter / gradient buffers fused_sgd.hip works
// on.  Three kernels per step:
//   flat_sumsq_partials  one per dtype group: per-block sum of squares of the
//                        gradient (fp32, fixed order, no atomics)
//   adamw_prepare        one block: folds all partials in double, advances the
//                        device-resident step counter, writes the bias
//                        corrections, the gradient norm and the clip coefficient
//   adamw_flat_step      one per dtype group: the update itself
// Step count, bias corrections and clip coefficient never leave the device, so
// step() has no host sync and a step captured into a hipGraph stays correct on
// replay (a host scalar would be frozen at capture).  lr is a host scalar, as
// in the SGD kernel.
//
// Every parameter's slot in a flat buffer is padded to 8 elements
// (ddp/reducer.cpp kAlignElems, MasterAdamW's layout), so an 8-element vector
// never straddles two parameters: the decay mask has one byte per vector.
//
// Semantics: torch.optim.AdamW(amsgrad=False, maximize=False) after
// torch.nn.utils.clip_grad_norm_.
//
// adamw_flat_step_scaled is adamw_flat_step with a per-tensor learning-rate
// scale (layer-wise lr decay for fine-tuning): still ONE launch per dtype
// group.  The scale rides the way the decay mask does: lr_class has one byte
// per 8-element vector and indexes lr_scales, an fp32 table of exactly 256
// entries -- any byte is in range, no bounds logic.  lr stays the host scalar
// the schedules write; class bytes and table stay on the device, so a step
// captured into a hipGraph reads the table of the replay, not of the capture.
//
// Per vector, s = lr_scales[lr_class[v]]:
//   s == 1   step_size = lr / bc1 and the host-formed decay, the scalars of
//            adamw_flat_kernel: the tensor gets that kernel's bits
//   else     lr_v = lr * s (fp32), step_size = lr_v / bc1, decay factor
//            fmaf(-lr_v, wd, 1): torch.optim.AdamW with lr = lr * s
//   s == 0   a frozen tensor: the moments update, the weights are stored back
//            as loaded (bit-unchanged even for -0.0 or a non-finite gradient)
//
// The table is staged into LDS once per block (1 KiB, one entry per thread):
// every lane then pays one ds_read_b32 per 28-byte-per-element vector.  Lanes
// of a wave mostly sit in one tensor, so the read is a broadcast.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "../api.h"
#include "../common.h"
#include "flat_step.h"

namespace dmp {
namespace {

constexpr int kClasses = 256;  // entries of lr_scales: one per value of a class byte
static_assert(kThreads == kClasses, "the table is staged one entry per thread");

// hyper[] slots (fp32, device)
constexpr int kBc1 = 0, kBc2 = 1, kNorm = 2, kClip = 3, kHyper = 4;

// Block b sums the squares of its grid-stride share of the vectors and writes
// out[b]; block 0 also zeroes the slots [gridDim.x, nslots) no block owns.
template <typename G>
__global__ __launch_bounds__(kThreads) void flat_sumsq_kernel(const G* __restrict__ grad, int64_t n,
                                                              float* __restrict__ out, int nslots) {
  __shared__ float red[kThreads / kWave];
  const int64_t nvec = n / 8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float acc = 0.f;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    float g[8];
    load8(grad + v * 8, g);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = fmaf(g[i], g[i], acc);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kThreads / kWave; ++i) s += red[i];
    out[blockIdx.x] = s;
  }
  if (blockIdx.x == 0)
    for (int i = gridDim.x + threadIdx.x; i < nslots; i += blockDim.x) out[i] = 0.f;
}

template <typename S>
__global__ __launch_bounds__(kThreads) void adamw_prepare_kernel(const float* __restrict__ partials,
                                                                 int64_t npart, float* __restrict__ hyper,
                                                                 S* __restrict__ step, double max_norm,
                                                                 double beta1, double beta2) {
  __shared__ double red[kThreads / kWave];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < npart; i += blockDim.x) acc += (double)partials[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
#pragma unroll
  for (int i = 0; i < kThreads / kWave; ++i) total += red[i];
  const S t = step[0] + 1;
  step[0] = t;
  hyper[kBc1] = (float)(1.0 - pow(beta1, (double)t));
  hyper[kBc2] = (float)(1.0 - pow(beta2, (double)t));
  if (partials != nullptr) {
    const double norm = sqrt(total);
    const double c = max_norm / (norm + 1e-6);
    hyper[kNorm] = (float)norm;
    hyper[kClip] = (float)(c > 1.0 ? 1.0 : c);  // a NaN norm stays NaN, as torch's clamp(max=1)
  } else {
    hyper[kNorm] = 0.f;
    hyper[kClip] = 1.f;
  }
}

template <typename G, typename P, bool MASTER, bool EMA>
__global__ __launch_bounds__(kThreads) void adamw_flat_kernel(
    float* __restrict__ master, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
    const G* __restrict__ grad, P* __restrict__ param, const uint8_t* __restrict__ decay_mask,
    const float* __restrict__ hyper, int64_t n, float lr, float beta1, float beta2, float omb1,
    float omb2, float eps, float decay, float* __restrict__ ema, float omd) {
  // uniform per-step scalars: one load each, then SGPR-resident
  const float clip = hyper[kClip];
  const float step_size = lr / hyper[kBc1];
  const float rsqrt_bc2 = 1.f / sqrtf(hyper[kBc2]);
  const int64_t nvec = n / 8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    const int64_t o = v * 8;
    float g[8], w[8], m[8], s[8];
    load8(grad + o, g);
    load_weights<MASTER>(master, param, o, w);
    load8(exp_avg + o, m);
    load8(exp_avg_sq + o, s);
    const float dk = (decay_mask == nullptr || decay_mask[v] != 0) ? decay : 1.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float gi = g[i] * clip;
      w[i] *= dk;
      m[i] = fmaf(beta1, m[i], omb1 * gi);
      s[i] = fmaf(beta2, s[i], omb2 * gi * gi);
      // sqrt(v) + eps, not m * rsqrt(v): an exactly-zero gradient history must give 0 / eps = 0
      const float denom = fmaf(sqrtf(s[i]), rsqrt_bc2, eps);
      w[i] = fmaf(-step_size, m[i] / denom, w[i]);
    }
    store8(exp_avg + o, m);
    store8(exp_avg_sq + o, s);
    store_weights<MASTER>(master, param, o, w);
    ema_update<EMA>(ema, o, w, omd);
  }
}

// adamw_flat_kernel with lr * lr_scales[lr_class[v]] as the learning rate of
// vector v.  The per-element update is adamw_flat_kernel's, a few lines up,
// line for line; a change there belongs here too
// (tests/test_gpu_layer_decay.py compares the bits).
template <typename G, typename P, bool MASTER, bool EMA>
__global__ __launch_bounds__(kThreads) void adamw_scaled_kernel(
    float* __restrict__ master, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
    const G* __restrict__ grad, P* __restrict__ param, const uint8_t* __restrict__ decay_mask,
    const float* __restrict__ hyper, const uint8_t* __restrict__ lr_class,
    const float* __restrict__ lr_scales, int64_t n, float lr, float beta1, float beta2, float omb1,
    float omb2, float eps, float decay, float wd, float* __restrict__ ema, float omd) {
  __shared__ float table[kClasses];
  table[threadIdx.x] = lr_scales[threadIdx.x];
  __syncthreads();
  // uniform per-step scalars: one load each, then SGPR-resident
  const float clip = hyper[kClip];
  const float bc1 = hyper[kBc1];
  const float step_uniform = lr / bc1;
  const float rsqrt_bc2 = 1.f / sqrtf(hyper[kBc2]);
  const int64_t nvec = n / 8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    const int64_t o = v * 8;
    float g[8], w[8], m[8], s[8];
    load8(grad + o, g);
    load_weights<MASTER>(master, param, o, w);
    load8(exp_avg + o, m);
    load8(exp_avg_sq + o, s);
    // (The mask load stays under its null test, after the 16-byte loads: hoisting both bytes above them
    // without a branch let the compiler sink half the 16-byte loads behind the stores, 4-6 % slower.)
    const float sc = table[lr_class[v]];
    const bool decays = decay_mask == nullptr || decay_mask[v] != 0;
    const bool unit = sc == 1.f, frozen = sc == 0.f;
    const float lr_v = lr * sc;
    const float step_size = unit ? step_uniform : lr_v / bc1;
    const float dk = decays ? (unit ? decay : fmaf(-lr_v, wd, 1.f)) : 1.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float gi = g[i] * clip;
      const float w0 = w[i];
      w[i] *= dk;
      m[i] = fmaf(beta1, m[i], omb1 * gi);
      s[i] = fmaf(beta2, s[i], omb2 * gi * gi);
      // sqrt(v) + eps, not m * rsqrt(v): an exactly-zero gradient history must give 0 / eps = 0
      const float denom = fmaf(sqrtf(s[i]), rsqrt_bc2, eps);
      w[i] = fmaf(-step_size, m[i] / denom, w[i]);
      w[i] = frozen ? w0 : w[i];
    }
    store8(exp_avg + o, m);
    store8(exp_avg_sq + o, s);
    store_weights<MASTER>(master, param, o, w);
    ema_update<EMA>(ema, o, w, omd);
  }
}

// A uint8 flat with one byte per 8-element vector of the step's flats (decay_mask, lr_class).
const uint8_t* check_vector_bytes(const at::Tensor& t, const char* name, const FlatStep& fs) {
  check_flat(t, name);
  TORCH_CHECK(t.scalar_type() == at::kByte && t.numel() == fs.n / 8 && t.get_device() == fs.dev, name,
              " must be uint8 [numel / 8] on the parameters' device");
  return t.data_ptr<uint8_t>();
}

// Both public steps: lr_class / lr_scales are null for adamw_flat_step.
void adamw_step(const c10::optional<at::Tensor>& master, at::Tensor& exp_avg, at::Tensor& exp_avg_sq,
                const at::Tensor& grad, at::Tensor& param, const c10::optional<at::Tensor>& decay_mask,
                const at::Tensor& hyper, const at::Tensor* lr_class, const at::Tensor* lr_scales, double lr,
                double beta1, double beta2, double eps, double weight_decay,
                const c10::optional<at::Tensor>& ema, double ema_decay) {
  const FlatStep fs = flat_step_args(master, grad, param, ema, ema_decay);
  float* m1 = check_flat_state(exp_avg, "exp_avg", fs);
  float* m2 = check_flat_state(exp_avg_sq, "exp_avg_sq", fs);
  check_flat(hyper, "hyper");
  TORCH_CHECK(hyper.scalar_type() == at::kFloat && hyper.numel() == kHyper && hyper.get_device() == fs.dev,
              "hyper must be fp32 [4] on the parameters' device");
  const float* hp = hyper.data_ptr<float>();
  const bool masked = decay_mask.has_value() && decay_mask->defined();
  const uint8_t* dm = masked ? check_vector_bytes(*decay_mask, "decay_mask", fs) : nullptr;
  const uint8_t* lc = nullptr;
  const float* ls = nullptr;
  if (lr_class != nullptr) {
    lc = check_vector_bytes(*lr_class, "lr_class", fs);
    check_flat(*lr_scales, "lr_scales");
    TORCH_CHECK(lr_scales->scalar_type() == at::kFloat && lr_scales->numel() == kClasses &&
                    lr_scales->get_device() == fs.dev,
                "lr_scales must be fp32 [256] on the parameters' device");
    ls = lr_scales->data_ptr<float>();
  }
  if (fs.n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid(flat_step_blocks(fs)), block(kThreads);
  // formed in double, rounded once: what torch's python-float hyper-parameters give
  const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  const float decay = (float)(1.0 - lr * weight_decay);
  dispatch_flat_step(fs, [&](auto g, auto p, auto m, auto e) {
    using G = decltype(g);
    using P = decltype(p);
    constexpr bool M = decltype(m)::value, E = decltype(e)::value;
    const G* gp = static_cast<const G*>(fs.grad);
    P* pp = static_cast<P*>(fs.param);
    if (lc != nullptr)
      hipLaunchKernelGGL((adamw_scaled_kernel<G, P, M, E>), grid, block, 0, stream, fs.master, m1, m2, gp, pp, dm,
                         hp, lc, ls, fs.n, (float)lr, (float)beta1, (float)beta2, omb1, omb2, (float)eps, decay,
                         (float)weight_decay, fs.ema, fs.omd);
    else
      hipLaunchKernelGGL((adamw_flat_kernel<G, P, M, E>), grid, block, 0, stream, fs.master, m1, m2, gp, pp, dm,
                         hp, fs.n, (float)lr, (float)beta1, (float)beta2, omb1, omb2, (float)eps, decay, fs.ema,
                         fs.omd);
  });
}

}  // namespace

int64_t adamw_grid_cap() { return kMaxBlocks; }

// grad: flat gradient (bf16 or fp32), numel a multiple of 8.  partials_row:
// fp32 [NB]; slot b < blocks holds block b's sum of squares, the rest zero.
void flat_sumsq_partials(const at::Tensor& grad, at::Tensor& partials_row) {
  check_flat(grad, "grad");
  check_flat(partials_row, "partials_row");
  TORCH_CHECK(partials_row.scalar_type() == at::kFloat && partials_row.numel() >= 1 &&
                  partials_row.numel() <= INT32_MAX,
              "partials_row must be a non-empty fp32 tensor");
  TORCH_CHECK(grad.get_device() == partials_row.get_device(), "grad / partials_row device mismatch");
  const int64_t n = grad.numel();
  TORCH_CHECK(n % 8 == 0, "flat buffers must be padded to a multiple of 8 elements");
  const bool gb = grad.scalar_type() == at::kBFloat16;
  TORCH_CHECK(gb || grad.scalar_type() == at::kFloat, "grad must be bf16 or fp32");
  const int nslots = (int)partials_row.numel();
  const int64_t nvec = n / 8;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((nvec + kThreads - 1) / kThreads, nslots));
  auto stream = at::hip::getCurrentHIPStream();
  float* out = partials_row.data_ptr<float>();
  if (gb)
    hipLaunchKernelGGL((flat_sumsq_kernel<__bf16>), dim3(blocks), dim3(kThreads), 0, stream,
                       reinterpret_cast<const __bf16*>(grad.data_ptr()), n, out, nslots);
  else
    hipLaunchKernelGGL((flat_sumsq_kernel<float>), dim3(blocks), dim3(kThreads), 0, stream,
                       grad.data_ptr<float>(), n, out, nslots);
}

// partials: fp32 [G, NB] of flat_sumsq_partials rows (undefined: clipping off).
// hyper: fp32 [4] = {1 - beta1^t, 1 - beta2^t, gradient norm, clip coefficient}.
// step: int32 / int64 [1], incremented here.
void adamw_prepare(const c10::optional<at::Tensor>& partials, at::Tensor& hyper, at::Tensor& step,
                   double max_norm, double beta1, double beta2) {
  check_flat(hyper, "hyper");
  check_flat(step, "step");
  TORCH_CHECK(hyper.scalar_type() == at::kFloat && hyper.numel() == kHyper, "hyper must be fp32 [4]");
  TORCH_CHECK(step.numel() == 1 && (step.scalar_type() == at::kInt || step.scalar_type() == at::kLong),
              "step must be a 1-element int32 / int64 tensor");
  TORCH_CHECK(step.get_device() == hyper.get_device(), "step / hyper device mismatch");
  const bool clip = max_norm > 0.0 && partials.has_value() && partials->defined();
  const float* pp = nullptr;
  int64_t npart = 0;
  if (clip) {
    check_flat(*partials, "partials");
    TORCH_CHECK(partials->scalar_type() == at::kFloat, "partials must be fp32");
    TORCH_CHECK(partials->get_device() == hyper.get_device(), "partials / hyper device mismatch");
    pp = partials->data_ptr<float>();
    npart = partials->numel();
  }
  auto stream = at::hip::getCurrentHIPStream();
  if (step.scalar_type() == at::kLong)
    hipLaunchKernelGGL((adamw_prepare_kernel<int64_t>), dim3(1), dim3(kThreads), 0, stream, pp, npart,
                       hyper.data_ptr<float>(), step.data_ptr<int64_t>(), max_norm, beta1, beta2);
  else
    hipLaunchKernelGGL((adamw_prepare_kernel<int32_t>), dim3(1), dim3(kThreads), 0, stream, pp, npart,
                       hyper.data_ptr<float>(), step.data_ptr<int32_t>(), max_norm, beta1, beta2);
}

// master: fp32 flat (or undefined when `param` is fp32 and is its own master)
// exp_avg / exp_avg_sq: fp32 flat moments; grad / param: bf16 or fp32 flats
// decay_mask: uint8 [numel / 8], one byte per 8-element vector (undefined:
// decay everywhere); hyper: as written by adamw_prepare.
// ema: fp32 flat average of the fp32 weights, ema += (1 - ema_decay) * (w - ema)
// in the same pass (undefined: none).
void adamw_flat_step(const c10::optional<at::Tensor>& master, at::Tensor& exp_avg, at::Tensor& exp_avg_sq,
                     const at::Tensor& grad, at::Tensor& param,
                     const c10::optional<at::Tensor>& decay_mask, const at::Tensor& hyper, double lr,
                     double beta1, double beta2, double eps, double weight_decay,
                     const c10::optional<at::Tensor>& ema, double ema_decay) {
  adamw_step(master, exp_avg, exp_avg_sq, grad, param, decay_mask, hyper, nullptr, nullptr, lr, beta1, beta2, eps,
             weight_decay, ema, ema_decay);
}

// adamw_flat_step with lr * lr_scales[lr_class[v]] as the learning rate of
// vector v.  lr_class: uint8 [numel / 8]; lr_scales: fp32 [256] (entries no
// class uses may hold anything).  Everything else as there.
void adamw_flat_step_scaled(const c10::optional<at::Tensor>& master, at::Tensor& exp_avg,
                            at::Tensor& exp_avg_sq, const at::Tensor& grad, at::Tensor& param,
                            const c10::optional<at::Tensor>& decay_mask, const at::Tensor& hyper,
                            const at::Tensor& lr_class, const at::Tensor& lr_scales, double lr, double beta1,
                            double beta2, double eps, double weight_decay,
                            const c10::optional<at::Tensor>& ema, double ema_decay) {
  adamw_step(master, exp_avg, exp_avg_sq, grad, param, decay_mask, hyper, &lr_class, &lr_scales, lr, beta1, beta2,
             eps, weight_decay, ema, ema_decay);
}

}  // namespace dmp
