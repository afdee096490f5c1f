// Host-side argument check of the optional weight EMA the three flat step
// kernels (fused_sgd.hip, fused_adamw.hip, fused_lars.hip) update in their own
// pass: ema += (1 - ema_decay) * (w - ema) over the fp32 weights just formed.
#pragma once

#include <torch/extension.h>

namespace dmp {

// The EMA's data pointer, or nullptr when there is none.
inline float* check_ema(const c10::optional<at::Tensor>& ema, double ema_decay,
                        const c10::optional<at::Tensor>& master, const at::Tensor& param) {
  if (!ema.has_value() || !ema->defined()) return nullptr;
  TORCH_CHECK(ema->is_cuda() && ema->is_contiguous() && ema->scalar_type() == at::kFloat,
              "ema must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(ema->get_device() == param.get_device() && ema->numel() == param.numel(),
              "ema must be an fp32 flat of the parameters' size on the parameters' device");
  TORCH_CHECK(ema_decay >= 0.0 && ema_decay < 1.0, "ema_decay must be in [0, 1), got ", ema_decay);
  TORCH_CHECK(!ema->is_alias_of(param), "ema must not share storage with param");
  if (master.has_value() && master->defined())
    TORCH_CHECK(!ema->is_alias_of(*master), "ema must not share storage with master");
  return ema->data_ptr<float>();
}

}  // namespace dmp
