// adamw_flat_step with a per-tensor learning-rate scale (layer-wise lr decay
// for fine-tuning): still ONE launch per dtype group over the flats of
// fused_adamw.hip.  The scale rides the way the decay mask does: lr_class has
// one byte per 8-element vector (a slot is padded to 8 elements, so a vector
// belongs to one tensor) and indexes lr_scales, an fp32 table of exactly 256
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
// The per-element update below is adamw_flat_kernel's, line for line; a change
// there belongs here too (tests/test_gpu_layer_decay.py compares the bits).
//
// The table is staged into LDS once per block (1 KiB, one entry per thread):
// every lane then pays one ds_read_b32 per 28-byte-per-element vector.  Lanes
// of a wave mostly sit in one tensor, so the read is a broadcast.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "../api.h"
#include "../common.h"
#include "ema.h"

namespace dmp {
namespace {

constexpr int kThreads = 256;
constexpr int kClasses = 256;  // entries of lr_scales: one per value of a class byte
static_assert(kThreads == kClasses, "the table is staged one entry per thread");

// hyper[] slots written by adamw_prepare (fused_adamw.hip)
constexpr int kBc1 = 0, kBc2 = 1, kClip = 3, kHyper = 4;

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
    if constexpr (MASTER) load8(master + o, w);
    else load8(reinterpret_cast<const float*>(param) + o, w);
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
    if constexpr (MASTER) store8(master + o, w);
    store8(param + o, w);
    if constexpr (EMA) {  // e += (1 - decay) * (w - e) on the fp32 weights just formed
      float e[8];
      load8(ema + o, e);
#pragma unroll
      for (int i = 0; i < 8; ++i) e[i] = fmaf(omd, w[i] - e[i], e[i]);
      store8(ema + o, e);
    }
  }
}

void check_flat(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name, " must be a contiguous GPU tensor");
}

}  // namespace

// adamw_flat_step (fused_adamw.hip) with lr * lr_scales[lr_class[v]] as the
// learning rate of vector v.  lr_class: uint8 [numel / 8]; lr_scales: fp32
// [256] (entries no class uses may hold anything).  Everything else as there.
void adamw_flat_step_scaled(const c10::optional<at::Tensor>& master, at::Tensor& exp_avg,
                            at::Tensor& exp_avg_sq, const at::Tensor& grad, at::Tensor& param,
                            const c10::optional<at::Tensor>& decay_mask, const at::Tensor& hyper,
                            const at::Tensor& lr_class, const at::Tensor& lr_scales, double lr, double beta1,
                            double beta2, double eps, double weight_decay,
                            const c10::optional<at::Tensor>& ema, double ema_decay) {
  const int64_t n = param.numel();
  check_flat(param, "param");
  check_flat(grad, "grad");
  check_flat(exp_avg, "exp_avg");
  check_flat(exp_avg_sq, "exp_avg_sq");
  check_flat(hyper, "hyper");
  check_flat(lr_class, "lr_class");
  check_flat(lr_scales, "lr_scales");
  TORCH_CHECK(grad.numel() == n && exp_avg.numel() == n && exp_avg_sq.numel() == n,
              "grad / moment / param size mismatch");
  TORCH_CHECK(n % 8 == 0, "flat buffers must be padded to a multiple of 8 elements");
  TORCH_CHECK(exp_avg.scalar_type() == at::kFloat && exp_avg_sq.scalar_type() == at::kFloat,
              "moments must be fp32");
  TORCH_CHECK(hyper.scalar_type() == at::kFloat && hyper.numel() == kHyper, "hyper must be fp32 [4]");
  const bool gb = grad.scalar_type() == at::kBFloat16, pb = param.scalar_type() == at::kBFloat16;
  TORCH_CHECK(gb || grad.scalar_type() == at::kFloat, "grad must be bf16 or fp32");
  TORCH_CHECK(pb || param.scalar_type() == at::kFloat, "param must be bf16 or fp32");
  const bool has_master = master.has_value() && master->defined();
  TORCH_CHECK(has_master || !pb, "bf16 parameters need an fp32 master buffer");
  const int dev = param.get_device();
  TORCH_CHECK(grad.get_device() == dev && exp_avg.get_device() == dev && exp_avg_sq.get_device() == dev &&
                  hyper.get_device() == dev, "all buffers must be on one device");
  TORCH_CHECK(lr_class.scalar_type() == at::kByte && lr_class.numel() == n / 8 && lr_class.get_device() == dev,
              "lr_class must be uint8 [numel / 8] on the parameters' device");
  TORCH_CHECK(lr_scales.scalar_type() == at::kFloat && lr_scales.numel() == kClasses &&
                  lr_scales.get_device() == dev,
              "lr_scales must be fp32 [256] on the parameters' device");
  float* mp = nullptr;
  if (has_master) {
    check_flat(*master, "master");
    TORCH_CHECK(master->scalar_type() == at::kFloat && master->numel() == n && master->get_device() == dev,
                "master must be an fp32 flat of the parameters' size");
    mp = master->data_ptr<float>();
  }
  const uint8_t* dm = nullptr;
  if (decay_mask.has_value() && decay_mask->defined()) {
    check_flat(*decay_mask, "decay_mask");
    TORCH_CHECK(decay_mask->scalar_type() == at::kByte && decay_mask->numel() == n / 8 &&
                    decay_mask->get_device() == dev, "decay_mask must be uint8 [numel / 8]");
    dm = decay_mask->data_ptr<uint8_t>();
  }
  float* ep = check_ema(ema, ema_decay, master, param);
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  const int64_t nvec = n / 8;
  const int64_t blocks = std::min<int64_t>((nvec + kThreads - 1) / kThreads, adamw_grid_cap());
  // formed in double, rounded once: what torch's python-float hyper-parameters give
  const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  const float decay = (float)(1.0 - lr * weight_decay);
  const float omd = (float)(1.0 - ema_decay);
  auto launch = [&](auto gtag, auto ptag) {
    using G = decltype(gtag);
    using P = decltype(ptag);
    const G* gp = reinterpret_cast<const G*>(grad.data_ptr());
    P* pp = reinterpret_cast<P*>(param.data_ptr());
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kThreads), 0, stream, mp, exp_avg.data_ptr<float>(),
                         exp_avg_sq.data_ptr<float>(), gp, pp, dm, hyper.data_ptr<float>(),
                         lr_class.data_ptr<uint8_t>(), lr_scales.data_ptr<float>(), n, (float)lr,
                         (float)beta1, (float)beta2, omb1, omb2, (float)eps, decay, (float)weight_decay, ep,
                         omd);
    };
    if (has_master) ep ? go(adamw_scaled_kernel<G, P, true, true>) : go(adamw_scaled_kernel<G, P, true, false>);
    else ep ? go(adamw_scaled_kernel<G, P, false, true>) : go(adamw_scaled_kernel<G, P, false, false>);
  };
  if (gb && pb) launch(__bf16{}, __bf16{});
  else if (gb) launch(__bf16{}, float{});
  else if (pb) launch(float{}, __bf16{});
  else launch(float{}, float{});
}

}  // namespace dmp
