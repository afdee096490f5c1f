// Fused binary cross-entropy over the classes (timm's BinaryCrossEntropy: the
// loss of the "ResNet strikes back" A1-A3 and DeiT-III recipes) for [B, C]
// logits in bf16 or fp32, with labels as indices.  The dense target timm builds,
//   d_c = e/C + (1-e) * (lam*[c==a] + (1-lam)*[c==b]),   t_c = th ? (d_c > th) : d_c,
// takes at most three values per row: t_u on every class, t_a at the first
// label a and t_b at the second label b.  They are computed once per row, so
//   loss_i = sum_c softplus(x_c) - t_u * sum_c x_c - (t_a - t_u) * x_a - (t_b - t_u) * x_b
//   dx_c   = (sigmoid(x_c) - t_c) * g * scale / norm
// need no [B, C] target, no fp32 copy of the logits and nothing saved but the
// three floats the reduce writes.  There is no row max and no log-sum-exp: one
// sweep per row forward, one backward.
//
// One wave64 per row.  A row is cut where its own address says so: a scalar
// head up to the first 16-byte boundary (at most 7 elements), 16-byte vectors
// (8 bf16 / 4 fp32 per lane and access), a scalar tail.  So a row stride or a
// view offset that is no multiple of 16 bytes (C = 365, a view one element into
// its allocation) still streams vectors, and a row shorter than a vector is all
// head and tail.  The backward writes dx [B, C] dense; it takes the same cut
// when every dx row has the alignment phase of its x row, else the scalar
// instantiation.  Sums are lane-ordered and tree-reduced: no atomics, the same
// bits every run.
//
// Conventions of cross_entropy.hip: a row is ignored iff its FIRST label is
// ignore_index; a label outside [0, C) on a valid row (ignore_index as a second
// label included) reads nothing and poisons that row with NaN.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "../api.h"
#include "../common.h"

namespace dmp {
namespace {

constexpr int kRowsPerBlock = 4;  // 4 waves, one row each

struct BceArgs {
  const int64_t* tgt_b;  // nullptr: one label per row
  float smooth;          // e
  float lam;
  float thresh;  // < 0: targets stay soft
  float per_row;  // norm = n_valid * per_row: C (timm's mean) or 1 (sum over the classes)
};

// (its own name: an overload here would hide common.h's wave_sum from this namespace)
__device__ __forceinline__ int wave_count(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The row's three target values (forward and backward take them from here, so
// they agree bit for bit).  same: both labels on one class, or no second label.
struct RowTargets {
  float u, a, b;  // every other class, the first label's class, the second label's class
};
__device__ __forceinline__ RowTargets row_targets(const BceArgs& p, int C, bool same) {
  const float off = p.smooth / (float)C, on = 1.f - p.smooth;
  RowTargets t{off, off + on * (same ? 1.f : p.lam), off + on * (1.f - p.lam)};
  if (p.thresh >= 0.f) {
    t.u = t.u > p.thresh ? 1.f : 0.f;
    t.a = t.a > p.thresh ? 1.f : 0.f;
    t.b = t.b > p.thresh ? 1.f : 0.f;
  }
  return t;
}

// Elements of the row before its first 16-byte boundary (all of a row that ends
// before it): the scalar head.  Fewer than a vector, so lanes 0..head-1 take it.
template <typename T>
__device__ __forceinline__ int row_head(const T* xr, int C) {
  return min(C, (int)((0 - reinterpret_cast<uintptr_t>(xr)) & 15) / (int)sizeof(T));
}

template <typename T, bool RANK>
__global__ __launch_bounds__(64 * kRowsPerBlock) void bce_fwd_kernel(
    const T* __restrict__ x, int64_t ldx, const int64_t* __restrict__ tgt, int B, int C,
    int64_t ignore_index, float* __restrict__ row_loss, int* __restrict__ rank_out, BceArgs p) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* xr = x + (int64_t)row * ldx;
  const int64_t a = tgt[row], b = p.tgt_b ? p.tgt_b[row] : a;
  const bool a_ok = a >= 0 && a < C, b_ok = b >= 0 && b < C;
  const float xa = a_ok ? (float)xr[a] : 0.f;
  float sp = 0.f, sx = 0.f;
  int r = 0;
  auto take = [&](float v, int c) {
    // softplus without overflow: max(x, 0) + log1p(exp(-|x|))
    sp += fmaxf(v, 0.f) + log1pf(__expf(-fabsf(v)));
    sx += v;
    // the first label's rank: classes ahead of it in a stable descending sort
    // (sigmoid is monotone, so by logit); top-k correct <=> rank < k
    if constexpr (RANK) r += (v > xa || (v == xa && c < a)) ? 1 : 0;
  };
  constexpr int N = Vec16<T>::N;
  const int head = row_head(xr, C), nv = (C - head) / N;
  if (lane < head) take((float)xr[lane], lane);
#pragma unroll 2
  for (int v = lane; v < nv; v += 64) {
    const int c0 = head + v * N;
    float e[N];
    Vec16<T>::load(xr + c0, e);
#pragma unroll
    for (int i = 0; i < N; ++i) take(e[i], c0 + i);
  }
  for (int c = head + nv * N + lane; c < C; c += 64) take((float)xr[c], c);
  sp = wave_sum(sp);
  sx = wave_sum(sx);
  if constexpr (RANK) {
    r = wave_count(r);
    if (lane == 0) rank_out[row] = a_ok ? r : C;
  }
  if (lane == 0) {
    float l = 0.f;
    if (a != ignore_index) {
      l = NAN;  // a label out of range reads nothing and poisons the row
      if (a_ok && b_ok) {
        const RowTargets t = row_targets(p, C, b == a);
        l = sp - t.u * sx - (t.a - t.u) * xa;
        if (b != a) l -= (t.b - t.u) * (float)xr[b];
      }
    }
    row_loss[row] = l;
  }
}

// loss = scale * sum(row_loss) / norm, norm = n_valid * per_row; writes (loss,
// norm, scale) for the backward; one block.  With ranks: acc (fp64 [3]) +=
// (loss, top-1 correct, top-kmax correct), as ce_reduce_kernel does.
__global__ __launch_bounds__(256) void bce_reduce_kernel(const float* __restrict__ row_loss,
                                                         const int64_t* __restrict__ tgt, int B,
                                                         int64_t ignore_index, float* __restrict__ out,
                                                         float scale, float per_row,
                                                         const int* __restrict__ rank, int kmax,
                                                         double* __restrict__ acc) {
  float s = 0.f, n = 0.f, c1 = 0.f, ck = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) {
    s += row_loss[i];
    n += tgt[i] != ignore_index ? 1.f : 0.f;
    if (rank) {
      c1 += rank[i] < 1 ? 1.f : 0.f;
      ck += rank[i] < kmax ? 1.f : 0.f;
    }
  }
  s = wave_sum(s);
  n = wave_sum(n);
  c1 = wave_sum(c1);
  ck = wave_sum(ck);
  __shared__ float rs[4], rn[4], r1[4], rk[4];
  if ((threadIdx.x & 63) == 0) {
    rs[threadIdx.x >> 6] = s;
    rn[threadIdx.x >> 6] = n;
    r1[threadIdx.x >> 6] = c1;
    rk[threadIdx.x >> 6] = ck;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float S = rs[0] + rs[1] + rs[2] + rs[3], N = rn[0] + rn[1] + rn[2] + rn[3];
    const float norm = N * per_row;
    const float L = N > 0.f ? S / norm * scale : NAN;  // zero valid rows: nan, as the cross-entropy
    out[0] = L;
    out[1] = norm;
    out[2] = scale;
    if (acc) {
      acc[0] += (double)L;
      acc[1] += (double)(r1[0] + r1[1] + r1[2] + r1[3]);
      acc[2] += (double)(rk[0] + rk[1] + rk[2] + rk[3]);
    }
  }
}

// sigmoid from z = exp(-|x|) in (0, 1]: nothing overflows
__device__ __forceinline__ float sigmoid(float v) {
  const float z = __expf(-fabsf(v));
  const float q = __builtin_amdgcn_rcpf(1.f + z);
  return v >= 0.f ? q : z * q;
}

// d loss / dx of class c, up to the row's factor k.  (A function of values: the
// same expression in a closure keeps the closure in memory, a target load per lane.)
__device__ __forceinline__ float bce_grad(float v, int c, int ca, int cb, RowTargets t, float k) {
  return (sigmoid(v) - (c == ca ? t.a : c == cb ? t.b : t.u)) * k;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(64 * kRowsPerBlock) void bce_bwd_kernel(
    const T* __restrict__ x, int64_t ldx, const int64_t* __restrict__ tgt, const float* __restrict__ gout,
    const float* __restrict__ stats, int B, int C, int64_t ignore_index, T* __restrict__ dx, BceArgs p) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* xr = x + (int64_t)row * ldx;
  T* dr = dx + (int64_t)row * C;
  const int64_t a = tgt[row], b = p.tgt_b ? p.tgt_b[row] : a;
  const bool bad = a < 0 || a >= C || b < 0 || b >= C;
  const float norm = stats[1];
  // ignored row (or no valid row at all): exactly zero; a label out of range: NaN
  const float k = (a == ignore_index || norm == 0.f) ? 0.f : bad ? NAN : gout[0] * stats[2] / norm;
  const RowTargets t = row_targets(p, C, b == a);
  // the class of each label as an int, -1 where it selects nothing (out of range: k is NaN or 0 anyway)
  const int ca = bad ? -1 : (int)a, cb = bad ? -1 : (int)b;
  if constexpr (VEC) {
    // dr has the alignment phase of xr (host check): one cut serves both
    constexpr int N = Vec16<T>::N;
    const int head = row_head(xr, C), nv = (C - head) / N;
    if (lane < head) dr[lane] = (T)bce_grad((float)xr[lane], lane, ca, cb, t, k);
#pragma unroll 2
    for (int v = lane; v < nv; v += 64) {
      const int c0 = head + v * N;
      float e[N];
      Vec16<T>::load(xr + c0, e);
#pragma unroll
      for (int i = 0; i < N; ++i) e[i] = bce_grad(e[i], c0 + i, ca, cb, t, k);
      Vec16<T>::store(dr + c0, e);
    }
    for (int c = head + nv * N + lane; c < C; c += 64) dr[c] = (T)bce_grad((float)xr[c], c, ca, cb, t, k);
  } else {
    for (int c = lane; c < C; c += 64) dr[c] = (T)bce_grad((float)xr[c], c, ca, cb, t, k);
  }
}

// Host checks shared by forward and backward, in the cross-entropy's wording.
BceArgs bce_args(const at::Tensor& x, const at::Tensor& target, double label_smoothing,
                 const c10::optional<at::Tensor>& target_b, double lam, const c10::optional<double>& target_thresh,
                 bool sum_classes) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.stride(1) == 1, "logits must be a row-major [B, C] GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, "logits must be fp32 or bf16");
  TORCH_CHECK(x.size(0) < (int64_t(1) << 31) && x.size(1) < (int64_t(1) << 31), "logits: batch or row too large");
  TORCH_CHECK(target.is_cuda() && target.device() == x.device() && target.scalar_type() == at::kLong &&
                  target.dim() == 1 && target.size(0) == x.size(0) && target.is_contiguous(),
              "target must be a contiguous int64 [B] GPU tensor");
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing < 1.0, "label_smoothing must be in [0, 1), got ",
              label_smoothing);
  TORCH_CHECK(lam >= 0.0 && lam <= 1.0, "lam must be in [0, 1], got ", lam);
  const bool has_b = target_b.has_value() && target_b->defined();
  if (has_b)
    TORCH_CHECK(target_b->is_cuda() && target_b->device() == x.device() && target_b->scalar_type() == at::kLong &&
                    target_b->dim() == 1 && target_b->size(0) == x.size(0) && target_b->is_contiguous(),
                "target_b must be a contiguous int64 [B] tensor on the logits' device");
  if (target_thresh.has_value())
    TORCH_CHECK(*target_thresh >= 0.0 && *target_thresh < 1.0, "target_thresh must be in [0, 1), got ",
                *target_thresh);
  BceArgs p;
  p.tgt_b = has_b ? target_b->data_ptr<int64_t>() : nullptr;
  p.smooth = (float)label_smoothing;
  p.lam = (float)lam;
  p.thresh = target_thresh.has_value() ? (float)*target_thresh : -1.f;
  p.per_row = sum_classes ? 1.f : (float)x.size(1);
  return p;
}

}  // namespace

// Returns (loss 0-d fp32, stats [3] fp32 = (loss, norm, scale)).  loss = scale *
// sum of the valid rows' BCE / norm, norm = n_valid * C, or n_valid with
// sum_classes.  acc (fp64 [3], optional): acc += (loss, top-1 correct,
// top-min(5, C) correct), ranked against the first label.
std::vector<at::Tensor> bce_fwd(const at::Tensor& x, const at::Tensor& target, int64_t ignore_index, double scale,
                                const c10::optional<at::Tensor>& acc, double label_smoothing,
                                const c10::optional<at::Tensor>& target_b, double lam,
                                const c10::optional<double>& target_thresh, bool sum_classes) {
  const BceArgs p = bce_args(x, target, label_smoothing, target_b, lam, target_thresh, sum_classes);
  const int B = (int)x.size(0), C = (int)x.size(1);
  auto fo = x.options().dtype(at::kFloat);
  const bool want = acc.has_value() && acc->defined();
  if (want)
    TORCH_CHECK(acc->is_cuda() && acc->device() == x.device() && acc->scalar_type() == at::kDouble &&
                    acc->numel() == 3 && acc->is_contiguous(),
                "bce_fwd: acc must be a contiguous fp64 [3] GPU tensor");
  auto row_loss = at::empty({B}, fo), stats = at::empty({3}, fo);
  at::Tensor rank;
  if (want) rank = at::empty({std::max(B, 1)}, x.options().dtype(at::kInt));
  int* rp = want ? rank.data_ptr<int>() : nullptr;
  auto stream = at::hip::getCurrentHIPStream();
  const int blocks = (B + kRowsPerBlock - 1) / kRowsPerBlock;
  auto launch = [&](auto ttag, auto rtag) {
    using T = decltype(ttag);
    hipLaunchKernelGGL((bce_fwd_kernel<T, decltype(rtag)::value>), dim3(blocks), dim3(64 * kRowsPerBlock), 0,
                       stream, reinterpret_cast<const T*>(x.data_ptr()), x.stride(0), target.data_ptr<int64_t>(),
                       B, C, ignore_index, row_loss.data_ptr<float>(), rp, p);
  };
  if (B > 0) {
    const bool f32 = x.scalar_type() == at::kFloat;
    if (f32 && want) launch(float{}, std::true_type{});
    else if (f32) launch(float{}, std::false_type{});
    else if (want) launch(__bf16{}, std::true_type{});
    else launch(__bf16{}, std::false_type{});
  }
  hipLaunchKernelGGL(bce_reduce_kernel, dim3(1), dim3(256), 0, stream, row_loss.data_ptr<float>(),
                     target.data_ptr<int64_t>(), B, ignore_index, stats.data_ptr<float>(), (float)scale, p.per_row,
                     B > 0 ? rp : nullptr, std::min(5, C), want ? acc->data_ptr<double>() : nullptr);
  DMP_HIP_CHECK(hipGetLastError());
  return {stats.select(0, 0), stats};
}

// d(logits) [B, C] dense, in the logits' dtype; stats is bce_fwd's second output.
at::Tensor bce_bwd(const at::Tensor& grad, const at::Tensor& x, const at::Tensor& target, const at::Tensor& stats,
                   int64_t ignore_index, double label_smoothing, const c10::optional<at::Tensor>& target_b,
                   double lam, const c10::optional<double>& target_thresh, bool sum_classes) {
  const BceArgs p = bce_args(x, target, label_smoothing, target_b, lam, target_thresh, sum_classes);
  TORCH_CHECK(stats.is_cuda() && stats.device() == x.device() && stats.scalar_type() == at::kFloat &&
                  stats.numel() == 3 && stats.is_contiguous(),
              "bce_bwd: stats must be the contiguous fp32 [3] tensor bce_fwd returned");
  TORCH_CHECK(grad.is_cuda() && grad.device() == x.device() && grad.numel() == 1,
              "bce_bwd: grad must be a one-element GPU tensor");
  const int B = (int)x.size(0), C = (int)x.size(1);
  auto g = grad.to(at::kFloat).contiguous();
  auto dx = at::empty({B, C}, x.options());
  if (B == 0 || C == 0) return dx;
  // one cut per row serves x and dx when their rows share the phase within 16 bytes
  const int64_t es = x.element_size();
  const bool vec = (reinterpret_cast<uintptr_t>(x.data_ptr()) - reinterpret_cast<uintptr_t>(dx.data_ptr())) % 16 == 0 &&
                   ((x.stride(0) - C) * es) % 16 == 0;
  auto stream = at::hip::getCurrentHIPStream();
  const int blocks = (B + kRowsPerBlock - 1) / kRowsPerBlock;
  auto launch = [&](auto ttag, auto vtag) {
    using T = decltype(ttag);
    hipLaunchKernelGGL((bce_bwd_kernel<T, decltype(vtag)::value>), dim3(blocks), dim3(64 * kRowsPerBlock), 0, stream,
                       reinterpret_cast<const T*>(x.data_ptr()), x.stride(0), target.data_ptr<int64_t>(),
                       g.data_ptr<float>(), stats.data_ptr<float>(), B, C, ignore_index,
                       reinterpret_cast<T*>(dx.data_ptr()), p);
  };
  const bool f32 = x.scalar_type() == at::kFloat;
  if (f32 && vec) launch(float{}, std::true_type{});
  else if (f32) launch(float{}, std::false_type{});
  else if (vec) launch(__bf16{}, std::true_type{});
  else launch(__bf16{}, std::false_type{});
  DMP_HIP_CHECK(hipGetLastError());
  return dx;
}

}  // namespace dmp
