// Single-launch SGD(momentum, weight decay, nesterov) over a FLAT parameter
// buffer: the whole model's parameters of one dtype live in one contiguous
// allocation laid out exactly like the DDP gradient buckets, so one kernel
// updates every parameter (ResNet-50: 25.6 M elements, ~1 launch instead of
// 161 per-tensor launches).  For bf16 models the kernel keeps fp32 master
// weights and momentum, reads the (already RCCL-averaged) bf16 gradient and
// writes the bf16 working copy back in the same pass -- no separate cast.
//
// Parity: the reference's optimizer is torch.optim.SGD(lr, momentum=0.9,
// weight_decay=1e-4) (model_parallel.py:105, data_parallel.py:90).
// Semantics match torch.optim.SGD exactly (first step seeds the buffer with
// the gradient, dampening applies from the second step on).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "../api.h"
#include "../common.h"
#include "flat_step.h"

namespace dmp {
namespace {

template <typename G, typename P, bool MASTER, bool EMA>
__global__ __launch_bounds__(kThreads) void sgd_flat_kernel(
    float* __restrict__ master, float* __restrict__ mom, const G* __restrict__ grad,
    P* __restrict__ param, int64_t n, float lr, float wd, float momentum, float dampening,
    int nesterov, float grad_scale, int first_step, float* __restrict__ ema, float omd) {
  // 8 elements per lane per iteration: bf16 grads/params = 16 B, fp32 = 2 x 16 B.
  const int64_t nvec = n / 8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    const int64_t o = v * 8;
    float g[8], w[8], m[8];
    load8(grad + o, g);
    load_weights<MASTER>(master, param, o, w);
    if (momentum != 0.f && !first_step) load8(mom + o, m);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float d = fmaf(wd, w[i], g[i] * grad_scale);
      if (momentum != 0.f) {
        m[i] = first_step ? d : fmaf(momentum, m[i], (1.f - dampening) * d);
        d = nesterov ? fmaf(momentum, m[i], d) : m[i];
      }
      w[i] = fmaf(-lr, d, w[i]);
    }
    if (momentum != 0.f) store8(mom + o, m);
    store_weights<MASTER>(master, param, o, w);
    ema_update<EMA>(ema, o, w, omd);
  }
}

}  // namespace

// master: fp32 flat (or undefined when `param` is fp32 and is its own master)
// mom:    fp32 flat momentum buffer (checked whatever `momentum` is; neither read nor written when it is 0)
// grad:   flat gradient (bf16 or fp32), param: flat parameters (bf16 or fp32)
// numel must be a multiple of 8 (bucket layouts are padded to 16 B).
// ema:    fp32 flat average of the fp32 weights, ema += (1 - ema_decay) * (w - ema)
//         in the same pass (undefined: none)
void sgd_flat_step(const c10::optional<at::Tensor>& master, at::Tensor& mom, const at::Tensor& grad,
                   at::Tensor& param, double lr, double wd, double momentum, double dampening, bool nesterov,
                   double grad_scale, bool first_step, const c10::optional<at::Tensor>& ema, double ema_decay) {
  const FlatStep fs = flat_step_args(master, grad, param, ema, ema_decay);
  float* mo = check_flat_state(mom, "mom", fs);
  if (fs.n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  dispatch_flat_step(fs, [&](auto g, auto p, auto m, auto e) {
    using G = decltype(g);
    using P = decltype(p);
    hipLaunchKernelGGL((sgd_flat_kernel<G, P, decltype(m)::value, decltype(e)::value>), dim3(flat_step_blocks(fs)),
                       dim3(kThreads), 0, stream, fs.master, mo, static_cast<const G*>(fs.grad),
                       static_cast<P*>(fs.param), fs.n, (float)lr, (float)wd, (float)momentum, (float)dampening,
                       (int)nesterov, (float)grad_scale, (int)first_step, fs.ema, fs.omd);
  });
}

}  // namespace dmp
