// Every native function the Python module binds from a .hip source, declared
// once, grouped by defining file.  bindings.cpp includes this header to bind
// them and each defining file includes it too, so a prototype that drifts from
// its definition fails in that file's own compile.  Host-only and torch-only:
// no HIP runtime header, usable from g++ and hipcc.  The launch helpers the
// .hip files share among themselves (they take a hipStream_t) are in launch.h;
// the classes have their own headers (comm/rccl_comm.h, ddp/reducer.h,
// dp/parallel_apply.h).
#pragma once

#include <ATen/ATen.h>
#include <c10/util/Optional.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace dmp {

// ---- attn/attention.hip ----
bool attention_supported(int64_t S, int64_t head_dim);
void set_attention_variant(int fwd, int bwd);
std::vector<int64_t> get_attention_variant();
void set_attention_long_from(int64_t n);
int64_t get_attention_long_from();
std::vector<at::Tensor> attention_forward(const at::Tensor& qkv, int64_t B, int64_t S, int64_t H, double scale);
at::Tensor attention_backward(const at::Tensor& dout, const at::Tensor& qkv, const at::Tensor& o,
                              const at::Tensor& lse, int64_t B, int64_t S, int64_t H, double scale);

// ---- bn/batchnorm.hip ----
at::Tensor bn_local_moments(const at::Tensor& x, int64_t C);
std::vector<at::Tensor> bn_forward_apply(const at::Tensor& x, const at::Tensor& sums,
                                         const c10::optional<at::Tensor>& weight,
                                         const c10::optional<at::Tensor>& bias,
                                         const c10::optional<at::Tensor>& running_mean,
                                         const c10::optional<at::Tensor>& running_var,
                                         double momentum, double eps,
                                         const c10::optional<at::Tensor>& residual, bool relu,
                                         int64_t C,
                                         const c10::optional<at::Tensor>& num_batches_tracked,
                                         bool out_moments, double clip);
std::vector<at::Tensor> bn_eval_apply(const at::Tensor& x, const at::Tensor& running_mean,
                                      const at::Tensor& running_var,
                                      const c10::optional<at::Tensor>& weight,
                                      const c10::optional<at::Tensor>& bias, double eps,
                                      const c10::optional<at::Tensor>& residual, bool relu,
                                      int64_t C, double clip);
at::Tensor bn_backward_moments(const at::Tensor& dy, const at::Tensor& x,
                               const c10::optional<at::Tensor>& y, const at::Tensor& mean,
                               bool relu, int64_t C, const c10::optional<at::Tensor>& weight,
                               const c10::optional<at::Tensor>& bias,
                               const c10::optional<at::Tensor>& invstd, double clip);
at::Tensor bn_finalize(const at::Tensor& sums, const c10::optional<at::Tensor>& weight,
                       const c10::optional<at::Tensor>& bias,
                       const c10::optional<at::Tensor>& running_mean,
                       const c10::optional<at::Tensor>& running_var, double momentum, double eps,
                       int64_t C, const c10::optional<at::Tensor>& num_batches_tracked);
std::vector<at::Tensor> bn_backward_apply(const at::Tensor& dy, const at::Tensor& x,
                                          const c10::optional<at::Tensor>& y,
                                          const at::Tensor& sums, const at::Tensor& count,
                                          const c10::optional<at::Tensor>& weight,
                                          const at::Tensor& mean, const at::Tensor& invstd,
                                          bool training, bool relu, bool want_dres, int64_t C,
                                          const c10::optional<at::Tensor>& bias, double clip,
                                          const c10::optional<at::Tensor>& acc_weight,
                                          const c10::optional<at::Tensor>& acc_bias);
void set_bn_streaming(bool on);
std::map<std::string, int64_t> bn_plan(int64_t M, int64_t C, at::ScalarType dtype);

// ---- bn/bn_apply_gram.hip ----
bool bn_apply_gram_supported(int64_t C);
std::vector<at::Tensor> bn_forward_apply_gram(const at::Tensor& x, const at::Tensor& sums,
                                              const c10::optional<at::Tensor>& weight,
                                              const c10::optional<at::Tensor>& bias,
                                              const c10::optional<at::Tensor>& running_mean,
                                              const c10::optional<at::Tensor>& running_var, double momentum,
                                              double eps, int64_t C,
                                              const c10::optional<at::Tensor>& num_batches_tracked, double clip);
void set_bn_gram_blocks(int64_t n);

// ---- bn/bn_fold.hip ----
bool bn_fold_supported(int64_t cout, int64_t cin);
std::vector<at::Tensor> bn_fold_fwd(const at::Tensor& W, const at::Tensor& G, const at::Tensor& asums,
                                    const c10::optional<at::Tensor>& Wf);
std::vector<at::Tensor> bn_fold_fwd_finalize(const at::Tensor& W, const at::Tensor& G, const at::Tensor& asums,
                                             const c10::optional<at::Tensor>& Wf,
                                             const c10::optional<at::Tensor>& weight,
                                             const c10::optional<at::Tensor>& bias,
                                             const c10::optional<at::Tensor>& running_mean,
                                             const c10::optional<at::Tensor>& running_var, double momentum,
                                             double eps, const c10::optional<at::Tensor>& num_batches_tracked);
at::Tensor bn_fold_bwd_sums(const at::Tensor& D, const at::Tensor& W, const at::Tensor& sdz,
                            const at::Tensor& mean);
std::vector<at::Tensor> bn_fold_bwd_coef(const at::Tensor& sums, const at::Tensor& local, const at::Tensor& count,
                                         const at::Tensor& invstd, const at::Tensor& mean,
                                         const c10::optional<at::Tensor>& gamma, const at::Tensor& D,
                                         const at::Tensor& WG, const at::Tensor& s, const at::Tensor& W);
std::vector<at::Tensor> bn_fold_relu_mask(const at::Tensor& dy, const at::Tensor& y);
at::Tensor bn_fold_colsum(const at::Tensor& x, const std::vector<int64_t>& map);
std::vector<at::Tensor> bn_fold_scale_concat(const at::Tensor& W3, const at::Tensor& s3, const at::Tensor& t3,
                                             const at::Tensor& Wd, const at::Tensor& sd, const at::Tensor& td);
void set_fold_gemm(int mode);
int get_fold_gemm();

// ---- comm/coalesced.hip ----
void multi_copy(const std::vector<at::Tensor>& srcs, const std::vector<at::Tensor>& dsts);
void multi_transpose(const std::vector<at::Tensor>& srcs, const std::vector<at::Tensor>& dsts,
                     const std::vector<int64_t>& taps);
void multi_cast_bf16_f32(const std::vector<at::Tensor>& srcs, const std::vector<at::Tensor>& dsts);
void reduce_add_into(const std::vector<at::Tensor>& inputs, at::Tensor& out);
void gather_slabs(const std::vector<at::Tensor>& inputs, at::Tensor& out, bool along_inner);
std::vector<std::vector<bool>> enable_peer_access(int64_t num_devices);

// ---- conv/conv3x3_c128.hip ----
std::vector<at::Tensor> conv3x3_c128(const at::Tensor& x, const at::Tensor& wmat, bool moments);
bool conv3x3_c128_supported(int64_t c, int64_t h, int64_t w);
at::Tensor conv3x3_c128_dgrad_s2(const at::Tensor& dy, const at::Tensor& wt);

// ---- conv/conv3x3_halo.hip ----
std::vector<at::Tensor> conv3x3_c64(const at::Tensor& x, const at::Tensor& wmat, bool moments);

// ---- conv/depthwise.hip ----
std::vector<at::Tensor> dwconv3x3_forward(const at::Tensor& x, const at::Tensor& w, int64_t stride,
                                          bool moments);
at::Tensor dwconv3x3_dgrad(const at::Tensor& dy, const at::Tensor& w, int64_t stride, int64_t H,
                           int64_t W);
at::Tensor dwconv3x3_wgrad(const at::Tensor& dy, const at::Tensor& x, int64_t stride,
                           at::ScalarType out_dtype, const c10::optional<at::Tensor>& out);
std::map<std::string, int64_t> dwconv3x3_plan(int64_t N, int64_t C, int64_t H, int64_t W, int64_t stride,
                                              at::ScalarType dtype);

// ---- conv/depthwise7.hip ----
at::Tensor dwconv7x7_forward(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias);
at::Tensor dwconv7x7_dgrad(const at::Tensor& dy, const at::Tensor& w, const c10::optional<at::Tensor>& add);
std::vector<at::Tensor> dwconv7x7_wgrad(const at::Tensor& dy, const at::Tensor& x, at::ScalarType w_dtype);
std::map<std::string, int64_t> dwconv7x7_plan(int64_t N, int64_t C, int64_t H, int64_t W);

// ---- conv/gemm_bf16.hip ----
std::vector<at::Tensor> gemm_nt(const at::Tensor& A, const at::Tensor& B,
                                const c10::optional<at::Tensor>& pro_scale,
                                const c10::optional<at::Tensor>& pro_shift, const std::string& mode,
                                const c10::optional<at::Tensor>& epi_scale,
                                const c10::optional<at::Tensor>& epi_shift,
                                const c10::optional<at::Tensor>& residual, bool relu,
                                const std::vector<int64_t>& a_map,
                                const std::vector<int64_t>& c_map,
                                const c10::optional<at::Tensor>& a2,
                                const std::vector<int64_t>& a2_map);
std::vector<at::Tensor> gemm_nt_bnbwd(const at::Tensor& A, const at::Tensor& B,
                                      const c10::optional<at::Tensor>& residual,
                                      const c10::optional<at::Tensor>& bn_x,
                                      const c10::optional<at::Tensor>& bn_y,
                                      const c10::optional<at::Tensor>& mean,
                                      const c10::optional<at::Tensor>& invstd,
                                      const c10::optional<at::Tensor>& weight,
                                      const c10::optional<at::Tensor>& bias,
                                      const std::vector<int64_t>& res_map,
                                      const c10::optional<at::Tensor>& a2,
                                      const c10::optional<at::Tensor>& ebias,
                                      const std::vector<int64_t>& a2_map);
at::Tensor gemm_tn(const at::Tensor& A, const at::Tensor& B, at::ScalarType out_dtype,
                   const std::vector<int64_t>& b_map, const c10::optional<at::Tensor>& pro_scale,
                   const c10::optional<at::Tensor>& pro_shift, bool a_mapped,
                   const c10::optional<at::Tensor>& out);
std::vector<at::Tensor> conv_nt(const at::Tensor& x, const at::Tensor& wmat, int64_t kh,
                                int64_t kw, int64_t stride, int64_t pad, int64_t ho, int64_t wo,
                                bool transposed, const c10::optional<at::Tensor>& pro_scale,
                                const c10::optional<at::Tensor>& pro_shift,
                                const std::string& mode,
                                const c10::optional<at::Tensor>& epi_scale,
                                const c10::optional<at::Tensor>& epi_shift,
                                const c10::optional<at::Tensor>& residual, bool relu,
                                int64_t kc);
at::Tensor conv_wgrad(const at::Tensor& dy, const at::Tensor& x, int64_t kh, int64_t kw,
                      int64_t stride, int64_t pad, int64_t ho, int64_t wo,
                      at::ScalarType out_dtype, int64_t kc, const c10::optional<at::Tensor>& out);
void set_gemm_tile(int64_t t);
void set_phase_dgrad(bool on);
void set_tn_wide(bool on);

// ---- conv/stem.hip ----
at::Tensor space_to_depth2(const at::Tensor& x, int64_t pad, int64_t out_channels);
at::Tensor pad_channels16(const at::Tensor& x, int64_t pad, int64_t extra_w);

// ---- conv/stem_halo.hip ----
bool stem_halo_supported(int64_t hs, int64_t ws, int64_t ho, int64_t wo);
std::vector<at::Tensor> stem_halo_fwd(const at::Tensor& s, const at::Tensor& wm, int64_t ho, bool moments);
at::Tensor stem_halo_wgrad(const at::Tensor& dy, const at::Tensor& s, int64_t ho, at::ScalarType out_dtype);
std::vector<at::Tensor> stem_halo_wgrad_pool(const at::Tensor& dy, const at::Tensor& idx, const at::Tensor& y,
                                             const at::Tensor& s, const at::Tensor& scale, const at::Tensor& shift,
                                             const at::Tensor& mean, int64_t ho, int64_t pad);
at::Tensor stem_fold_finish(const at::Tensor& img, int64_t ho, int64_t wo, const at::Tensor& t_dz,
                            const at::Tensor& t_y, const at::Tensor& sums, const at::Tensor& cnt,
                            const at::Tensor& invstd, const c10::optional<at::Tensor>& weight, const at::Tensor& mean,
                            at::ScalarType out_dtype);

// ---- conv/wgrad3x3.hip ----
at::Tensor wgrad3x3(const at::Tensor& dy, const at::Tensor& x, int64_t stride);
bool wgrad3x3_supported(int64_t C, int64_t H, int64_t W, int64_t stride);
void set_wgrad3x3_waves(int64_t nw);

// ---- data/augment.hip ----
at::Tensor augment_batch(const at::Tensor& src, const at::Tensor& plan, int64_t out_h, int64_t out_w,
                         const std::vector<double>& mean, const std::vector<double>& std_, at::ScalarType dtype,
                         bool channels_last, bool no_resize);

// ---- data/rand_augment.hip ----
at::Tensor crop_bytes(const at::Tensor& src, const at::Tensor& plan, int64_t out_h, int64_t out_w);
at::Tensor rand_augment_apply(const at::Tensor& u8, const at::Tensor& ops, const at::Tensor& args,
                              const std::vector<int64_t>& hist_slots, const std::vector<int64_t>& fill,
                              const at::Tensor& table, at::ScalarType dtype, bool channels_last);

// ---- data/random_erase.hip ----
void random_erase(const at::Tensor& x, const at::Tensor& boxes, const c10::optional<at::Tensor>& fill, bool noise);
at::Tensor philox_bits(const at::Tensor& counters, const at::Tensor& key);

// ---- data/batch_mix.hip ----
at::Tensor batch_mix(const at::Tensor& x, const at::Tensor& perm, double lam, const std::vector<int64_t>& box);

// ---- gemm/gemm_xl.hip (NT: host side; kernels in gemm_xl_nt8.hip, gemm_xl_w4.hip, gemm_xl_x2.hip) ----
at::Tensor gemm_xl(const at::Tensor& A, const at::Tensor& B, const std::string& mode,
                   const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& aux,
                   const c10::optional<at::Tensor>& residual, const c10::optional<at::Tensor>& out,
                   const c10::optional<at::Tensor>& row_scale = c10::nullopt, int64_t rows_per_sample = 0);
std::vector<at::Tensor> gemm_xl_dgelu_bgrad(const at::Tensor& A, const at::Tensor& B, const at::Tensor& aux);
std::vector<at::Tensor> gemm_xl_conv(const at::Tensor& A, const at::Tensor& B, const std::string& mode,
                                     const c10::optional<at::Tensor>& residual,
                                     const c10::optional<at::Tensor>& bn_x,
                                     const c10::optional<at::Tensor>& bn_y,
                                     const c10::optional<at::Tensor>& mean,
                                     const c10::optional<at::Tensor>& invstd,
                                     const c10::optional<at::Tensor>& weight,
                                     const c10::optional<at::Tensor>& bias,
                                     const std::vector<int64_t>& res_map,
                                     const c10::optional<at::Tensor>& a2,
                                     const c10::optional<at::Tensor>& ebias,
                                     const c10::optional<at::Tensor>& scale,
                                     const c10::optional<at::Tensor>& shift, bool relu,
                                     const std::vector<int64_t>& a2_map);
std::vector<at::Tensor> conv_xl(const at::Tensor& x, const at::Tensor& wmat, int64_t kh, int64_t kw,
                                int64_t stride, int64_t pad, int64_t ho, int64_t wo, const std::string& mode,
                                const c10::optional<at::Tensor>& residual, const c10::optional<at::Tensor>& bn_x,
                                const c10::optional<at::Tensor>& bn_y, const c10::optional<at::Tensor>& mean,
                                const c10::optional<at::Tensor>& invstd, const c10::optional<at::Tensor>& weight,
                                const c10::optional<at::Tensor>& bias);
at::Tensor conv_xl_dgrad_s2(const at::Tensor& dy, const std::vector<at::Tensor>& wph, int64_t hi, int64_t wi);
void set_gemm_xl_bn(int bn, int pipe, int group_m);
int get_gemm_xl_pipe();  // the one pipe selection; gemm_tn_xl.hip reads it through this
void set_gemm_xl_x2(int mode);
int get_gemm_xl_x2();
void set_gemm_xl_bm(int bm);
int get_gemm_xl_bm(int64_t M, int64_t N, int64_t K);
void set_gemm_xl_trace(const c10::optional<at::Tensor>& buf);
void set_gemm_xl_trim_heavy(bool on);

// ---- gemm/gemm_tn_xl.hip (TN) ----
at::Tensor gemm_tn_xl(const at::Tensor& A, const at::Tensor& B, at::ScalarType out_dtype,
                      const c10::optional<at::Tensor>& out);
at::Tensor gram_strided_xl(const at::Tensor& x, int64_t stride, int64_t ho, int64_t wo);
bool gram_strided_xl_supported(int64_t nb, int64_t cin, int64_t hi, int64_t wi, int64_t ho, int64_t wo);
at::Tensor conv_wgrad_xl(const at::Tensor& dy, const at::Tensor& x, int64_t kh, int64_t kw, int64_t stride,
                         int64_t pad, int64_t ho, int64_t wo, at::ScalarType out_dtype,
                         const c10::optional<at::Tensor>& out);
void set_tn_xl_rounds(int r);
void set_tn_narrow(bool on);

// ---- linear/bias_act.hip ----
bool colsum_supported(int64_t N);
at::Tensor bias_grad(const at::Tensor& dy, at::ScalarType out_dtype);
std::vector<at::Tensor> gelu_bwd_bias_grad(const at::Tensor& dy, const at::Tensor& h, at::ScalarType out_dtype);
std::vector<at::Tensor> rowscale_bias_grad(const at::Tensor& dy, const at::Tensor& row_scale, int64_t rows_per_sample,
                                           at::ScalarType out_dtype);

// ---- loss/cross_entropy.hip ----
std::vector<at::Tensor> cross_entropy_fwd(const at::Tensor& x, const at::Tensor& target,
                                          int64_t ignore_index, double scale,
                                          const c10::optional<at::Tensor>& acc, double label_smoothing,
                                          const c10::optional<at::Tensor>& target_b, double lam);
at::Tensor cross_entropy_bwd(const at::Tensor& grad, const at::Tensor& x, const at::Tensor& target,
                             const at::Tensor& lse, const at::Tensor& stats, int64_t ignore_index,
                             double label_smoothing, const c10::optional<at::Tensor>& target_b, double lam);
// ---- norm/layernorm.hip ----
std::vector<at::Tensor> layernorm_forward(const at::Tensor& x, const c10::optional<at::Tensor>& w,
                                          const c10::optional<at::Tensor>& b, int64_t D,
                                          double eps);
std::vector<at::Tensor> layernorm_backward(const at::Tensor& dy, const at::Tensor& x,
                                           const c10::optional<at::Tensor>& w,
                                           const at::Tensor& mean, const at::Tensor& rstd,
                                           int64_t D, at::ScalarType param_dtype,
                                           const c10::optional<at::Tensor>& dres);
bool layernorm_supported(int64_t D);

// ---- optim/fused_adamw.hip ----
void flat_sumsq_partials(const at::Tensor& grad, at::Tensor& partials_row);
void adamw_prepare(const c10::optional<at::Tensor>& partials, at::Tensor& hyper, at::Tensor& step,
                   double max_norm, double beta1, double beta2);
void adamw_flat_step(const c10::optional<at::Tensor>& master, at::Tensor& exp_avg, at::Tensor& exp_avg_sq,
                     const at::Tensor& grad, at::Tensor& param,
                     const c10::optional<at::Tensor>& decay_mask, const at::Tensor& hyper, double lr,
                     double beta1, double beta2, double eps, double weight_decay,
                     const c10::optional<at::Tensor>& ema, double ema_decay);
int64_t adamw_grid_cap();  // most blocks adamw_flat_step launches (256 threads, 8 elements each)
void adamw_flat_step_scaled(const c10::optional<at::Tensor>& master, at::Tensor& exp_avg,
                            at::Tensor& exp_avg_sq, const at::Tensor& grad, at::Tensor& param,
                            const c10::optional<at::Tensor>& decay_mask, const at::Tensor& hyper,
                            const at::Tensor& lr_class, const at::Tensor& lr_scales, double lr, double beta1,
                            double beta2, double eps, double weight_decay,
                            const c10::optional<at::Tensor>& ema, double ema_decay);

// ---- optim/fused_lars.hip ----
void lars_norm_partials(const c10::optional<at::Tensor>& master, const at::Tensor& grad,
                        const at::Tensor& param, const at::Tensor& items, at::Tensor& partials);
void lars_trust(const at::Tensor& partials, const at::Tensor& tensors, at::Tensor& coef,
                double trust_coefficient, double weight_decay, double eps);
void lars_flat_step(const c10::optional<at::Tensor>& master, at::Tensor& mom, const at::Tensor& grad,
                    at::Tensor& param, const at::Tensor& items, const at::Tensor& coef, double lr,
                    double momentum, const c10::optional<at::Tensor>& ema, double ema_decay);
int64_t lars_chunk_elems();   // most elements of one work item (one block of the norm / update kernels)
int64_t lars_fold_threads();  // lanes that fold one tensor's partials in lars_trust

// ---- optim/fused_sgd.hip ----
void sgd_flat_step(const c10::optional<at::Tensor>& master, at::Tensor& mom, const at::Tensor& grad,
                   at::Tensor& param, double lr, double wd, double momentum, double dampening, bool nesterov,
                   double grad_scale, bool first_step, const c10::optional<at::Tensor>& ema, double ema_decay);

// ---- pool/maxpool.hip ----
std::vector<at::Tensor> maxpool2d_forward(const at::Tensor& x, int64_t k, int64_t s, int64_t p);
at::Tensor maxpool2d_backward(const at::Tensor& dy, const at::Tensor& idx, int64_t H, int64_t W,
                              int64_t k, int64_t s, int64_t p);
at::Tensor global_avgpool_backward(const at::Tensor& g, int64_t H, int64_t W);
// fused stem BN + pool
std::vector<at::Tensor> maxpool2d_bn_forward(const at::Tensor& x, const at::Tensor& scale,
                                             const at::Tensor& shift, int64_t k, int64_t s, int64_t p);
std::vector<at::Tensor> maxpool2d_bn_backward(const at::Tensor& dy, const at::Tensor& idx, const at::Tensor& x,
                                              const at::Tensor& scale, const at::Tensor& shift,
                                              const at::Tensor& mean, int64_t k, int64_t s, int64_t p);
void set_pool_generic(bool on);

}  // namespace dmp
