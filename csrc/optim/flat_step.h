// What the flat step kernels (fused_sgd.hip, fused_adamw.hip, fused_lars.hip)
// share.  Host side: the argument checks of one step over the flats of a dtype
// group, the choice of the kernel's <G, P, MASTER, EMA> instantiation and the
// grid-stride grid.  Device side: the weights in and out, and the optional
// weight EMA every step kernel updates in its own pass,
// ema += (1 - ema_decay) * (w - ema) over the fp32 weights just formed.
#pragma once

#include <torch/extension.h>

#include <algorithm>
#include <type_traits>

#include "../common.h"

namespace dmp {

constexpr int kThreads = 256;        // block size of every kernel in csrc/optim
constexpr int kMaxBlocks = 256 * 8;  // grid cap of the grid-stride step kernels (sgd_flat_step, adamw_flat_step)

inline void check_flat(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name, " must be a contiguous GPU tensor");
}

// The checked arguments every step entry point has.
struct FlatStep {
  int64_t n = 0;  // elements of every flat, a multiple of 8
  int dev = 0;
  bool grad_bf16 = false, param_bf16 = false, has_master = false;
  float* master = nullptr;  // nullptr: fp32 parameters that are their own master
  float* ema = nullptr;     // nullptr: no EMA
  float omd = 0.f;          // 1 - ema_decay
  const void* grad = nullptr;
  void* param = nullptr;

  // the fp32 weights the update reads
  const float* weights() const { return has_master ? master : static_cast<const float*>(param); }
};

// master: fp32 flat (undefined: `param` is fp32 and its own master); grad /
// param: bf16 or fp32 flats of one size, a multiple of 8; ema: fp32 flat that
// shares no storage with the weights (undefined: none), ema_decay in [0, 1).
inline FlatStep flat_step_args(const c10::optional<at::Tensor>& master, const at::Tensor& grad,
                               const at::Tensor& param, const c10::optional<at::Tensor>& ema,
                               double ema_decay) {
  FlatStep fs;
  check_flat(param, "param");
  check_flat(grad, "grad");
  fs.n = param.numel();
  fs.dev = param.get_device();
  TORCH_CHECK(grad.numel() == fs.n && grad.get_device() == fs.dev, "grad / param size or device mismatch");
  TORCH_CHECK(fs.n % 8 == 0, "flat buffers must be padded to a multiple of 8 elements");
  fs.grad_bf16 = grad.scalar_type() == at::kBFloat16;
  fs.param_bf16 = param.scalar_type() == at::kBFloat16;
  TORCH_CHECK(fs.grad_bf16 || grad.scalar_type() == at::kFloat, "grad must be bf16 or fp32");
  TORCH_CHECK(fs.param_bf16 || param.scalar_type() == at::kFloat, "param must be bf16 or fp32");
  fs.has_master = master.has_value() && master->defined();
  TORCH_CHECK(fs.has_master || !fs.param_bf16, "bf16 parameters need an fp32 master buffer");
  if (fs.has_master) {
    check_flat(*master, "master");
    TORCH_CHECK(master->scalar_type() == at::kFloat && master->numel() == fs.n && master->get_device() == fs.dev,
                "master must be an fp32 flat of the parameters' size on the parameters' device");
    fs.master = master->data_ptr<float>();
  }
  if (ema.has_value() && ema->defined()) {
    TORCH_CHECK(ema->is_cuda() && ema->is_contiguous() && ema->scalar_type() == at::kFloat,
                "ema must be a contiguous fp32 GPU tensor");
    TORCH_CHECK(ema->get_device() == fs.dev && ema->numel() == fs.n,
                "ema must be an fp32 flat of the parameters' size on the parameters' device");
    TORCH_CHECK(ema_decay >= 0.0 && ema_decay < 1.0, "ema_decay must be in [0, 1), got ", ema_decay);
    TORCH_CHECK(!ema->is_alias_of(param), "ema must not share storage with param");
    TORCH_CHECK(!fs.has_master || !ema->is_alias_of(*master), "ema must not share storage with master");
    fs.ema = ema->data_ptr<float>();
  }
  fs.omd = (float)(1.0 - ema_decay);  // formed in double, rounded once
  fs.grad = grad.data_ptr();
  fs.param = param.data_ptr();
  return fs;
}

// An fp32 state flat (momentum, exp_avg, exp_avg_sq) of the step's size on its device.
inline float* check_flat_state(at::Tensor& t, const char* name, const FlatStep& fs) {
  check_flat(t, name);
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.numel() == fs.n && t.get_device() == fs.dev, name,
              " must be an fp32 flat of the parameters' size on the parameters' device");
  return t.data_ptr<float>();
}

// f(G{}, P{}, std::bool_constant<MASTER>{}, std::bool_constant<EMA>{}) for the
// step's dtypes and buffers: the one place that picks a step kernel's instantiation.
template <typename F>
void dispatch_flat_step(const FlatStep& fs, F&& f) {
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  auto flags = [&](auto g, auto p) {
    if (fs.has_master) fs.ema ? f(g, p, yes, yes) : f(g, p, yes, no);
    else fs.ema ? f(g, p, no, yes) : f(g, p, no, no);
  };
  if (fs.grad_bf16 && fs.param_bf16) flags(__bf16{}, __bf16{});
  else if (fs.grad_bf16) flags(__bf16{}, float{});
  else if (fs.param_bf16) flags(float{}, __bf16{});
  else flags(float{}, float{});
}

// Blocks of a grid-stride step kernel: one 8-element vector per lane and pass.
inline unsigned flat_step_blocks(const FlatStep& fs) {
  return (unsigned)std::min<int64_t>((fs.n / 8 + kThreads - 1) / kThreads, kMaxBlocks);
}

// ---- device: 8 fp32 weights at element o in and out, and the EMA that follows them ----
template <bool MASTER, typename P>
__device__ __forceinline__ void load_weights(const float* __restrict__ master, const P* __restrict__ param,
                                             int64_t o, float (&w)[8]) {
  if constexpr (MASTER) load8(master + o, w);
  else load8(reinterpret_cast<const float*>(param) + o, w);
}

template <bool MASTER, typename P>
__device__ __forceinline__ void store_weights(float* __restrict__ master, P* __restrict__ param, int64_t o,
                                              const float (&w)[8]) {
  if constexpr (MASTER) store8(master + o, w);
  store8(param + o, w);
}

template <bool EMA>
__device__ __forceinline__ void ema_update(float* __restrict__ ema, int64_t o, const float (&w)[8], float omd) {
  if constexpr (EMA) {  // e += (1 - decay) * (w - e) on the fp32 weights just formed
    float e[8];
    load8(ema + o, e);
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = fmaf(omd, w[i] - e[i], e[i]);
    store8(ema + o, e);
  }
}

}  // namespace dmp
