// Batch mixing for mixup / CutMix over a channels-last image batch [B, C, H, W]
// (bf16 or fp32), one launch, out of place (row i reads row perm[i], which
// another block may be writing):
//   mixup  (no box):              out[i] = lam * x[i] + (1 - lam) * x[perm[i]]
//                                 in fp32, rounded once to the dtype
//   CutMix (box = y0, y1, x0, x1): out[i] = x[perm[i]] inside the half-open
//                                 box, x[i] outside -- a pure copy, bit for bit
// instead of a gather, two scalings and an add (or a gather and a strided
// copy) over the whole input batch.
//
// A sample is one dense run of n = H*W*C elements.  When n is a multiple of the
// 16-byte vector and both bases are 16-byte aligned every sample base is
// aligned too and each lane moves 16 bytes per access; otherwise the scalar
// instantiation runs.  With C = 3 a vector straddles pixels, so the in-box
// test is per element: a lane decodes (y, x, c) of its first element once and
// walks the rest with carries.  A CutMix lane loads x[perm[i]] only when one of
// its elements is inside the box and x[i] only when one is outside, so the
// traffic stays near 2 x the tensor.  A perm[i] outside [0, B) reads nothing
// and writes row i as NaN.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "../api.h"
#include "../common.h"

namespace dmp {
namespace {

using u16x8 = uint16_t __attribute__((ext_vector_type(8)));

// The 16-byte vector of T as integers (a copy must not touch the bits).
template <typename T> struct Bits;
template <> struct Bits<float> {
  using E = uint32_t;
  using raw = u32x4;
  static constexpr int N = 4;
  static constexpr E kNaN = 0x7fc00000u;
};
template <> struct Bits<__bf16> {
  using E = uint16_t;
  using raw = u16x8;
  static constexpr int N = 8;
  static constexpr E kNaN = 0x7fc0u;
};

struct MixBox {
  int y0, y1, x0, x1;
};

constexpr int kThreads = 256;

// lam * a + oml * b with a rounding after each multiply and after the add (no
// fused multiply-add): the fp32 value is that of the PyTorch expression bit for bit.
__device__ __forceinline__ float mix2(float lam, float a, float oml, float b) {
#pragma clang fp contract(off)
  return lam * a + oml * b;
}

// grid: x = chunks of one sample (grid-stride over its vectors), y = samples
// (grid-stride over the batch).  n < 2^31 (host check), so element indices
// within a sample are 32-bit; sample bases are 64-bit.
template <typename T, bool CUT, bool VEC>
__global__ __launch_bounds__(kThreads) void batch_mix_kernel(
    const T* __restrict__ x, const int64_t* __restrict__ perm, T* __restrict__ out, int B, int n, int C,
    int W, float lam, float oml, MixBox box) {
  using BT = Bits<T>;
  using E = typename BT::E;
  using R = typename BT::raw;
  constexpr int N = VEC ? BT::N : 1;
  const int nv = n / N;  // VEC: n % N == 0
  const int step = gridDim.x * kThreads;
  for (int i = blockIdx.y; i < B; i += gridDim.y) {
    const int64_t p = perm[i];
    const E* xa = reinterpret_cast<const E*>(x) + (int64_t)i * n;
    E* o = reinterpret_cast<E*>(out) + (int64_t)i * n;
    if (p < 0 || p >= B) {  // block-uniform: hostile index, nothing read
      for (int v = blockIdx.x * kThreads + threadIdx.x; v < nv; v += step) {
        if constexpr (VEC) {
          R r;
#pragma unroll
          for (int k = 0; k < N; ++k) r[k] = BT::kNaN;
          *reinterpret_cast<R*>(o + (int64_t)v * N) = r;
        } else {
          o[v] = BT::kNaN;
        }
      }
      continue;
    }
    const E* xb = reinterpret_cast<const E*>(x) + p * n;
    for (int v = blockIdx.x * kThreads + threadIdx.x; v < nv; v += step) {
      const int e0 = v * N;
      if constexpr (CUT) {
        // (y, xw, c) of element e0 in the NHWC sample
        const unsigned pix = (unsigned)e0 / (unsigned)C;
        int c = e0 - (int)pix * C;
        int y = (int)(pix / (unsigned)W);
        int xw = (int)pix - y * W;
        bool in[N];
        bool any = false, all = true;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          in[k] = y >= box.y0 && y < box.y1 && xw >= box.x0 && xw < box.x1;
          any |= in[k];
          all &= in[k];
          if (++c == C) {
            c = 0;
            if (++xw == W) {
              xw = 0;
              ++y;
            }
          }
        }
        if constexpr (VEC) {
          R a = {}, b = {}, r;
          if (!all) a = *reinterpret_cast<const R*>(xa + e0);
          if (any) b = *reinterpret_cast<const R*>(xb + e0);
#pragma unroll
          for (int k = 0; k < N; ++k) r[k] = in[k] ? b[k] : a[k];
          *reinterpret_cast<R*>(o + e0) = r;
        } else {
          o[e0] = in[0] ? xb[e0] : xa[e0];
        }
      } else {
        const T* ta = reinterpret_cast<const T*>(xa) + e0;
        const T* tb = reinterpret_cast<const T*>(xb) + e0;
        T* to = reinterpret_cast<T*>(o) + e0;
        // the fp32 expression lam * a + (1 - lam) * b (mix2), then one rounding to T
        if constexpr (VEC) {
          float a[N], b[N], r[N];
          Vec16<T>::load(ta, a);
          Vec16<T>::load(tb, b);
#pragma unroll
          for (int k = 0; k < N; ++k) r[k] = mix2(lam, a[k], oml, b[k]);
          Vec16<T>::store(to, r);
        } else {
          *to = (T)mix2(lam, (float)*ta, oml, (float)*tb);
        }
      }
    }
  }
}

}  // namespace

// x: dense channels-last [B, C, H, W] bf16 / fp32; perm: int64 [B] on x's device;
// box: empty (mixup with lam) or [y0, y1, x0, x1] half-open (CutMix, lam unused).
at::Tensor batch_mix(const at::Tensor& x, const at::Tensor& perm, double lam, const std::vector<int64_t>& box) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "batch_mix: x must be a 4-D GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, "batch_mix: x must be fp32 or bf16");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), "batch_mix: x must be dense channels-last");
  const int64_t B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(perm.is_cuda() && perm.device() == x.device() && perm.scalar_type() == at::kLong && perm.dim() == 1 &&
                  perm.size(0) == B && perm.is_contiguous(),
              "batch_mix: perm must be a contiguous int64 [B] tensor on x's device");
  TORCH_CHECK(box.empty() || box.size() == 4, "batch_mix: box must be empty or [y0, y1, x0, x1]");
  const bool cut = !box.empty();
  MixBox mb{0, 0, 0, 0};
  if (cut) {
    TORCH_CHECK(0 <= box[0] && box[0] <= box[1] && box[1] <= H && 0 <= box[2] && box[2] <= box[3] && box[3] <= W,
                "batch_mix: box must satisfy 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W");
    mb = MixBox{(int)box[0], (int)box[1], (int)box[2], (int)box[3]};
  } else {
    TORCH_CHECK(lam >= 0.0 && lam <= 1.0, "batch_mix: lam must be in [0, 1], got ", lam);
  }
  const int64_t n = C * H * W;
  TORCH_CHECK(n < (int64_t(1) << 31) && B < (int64_t(1) << 31), "batch_mix: sample or batch too large");
  auto out = at::empty_strided(x.sizes(), x.strides(), x.options());
  if (B == 0 || n == 0) return out;
  const int64_t nvec16 = 16 / x.element_size();
  const bool vec = n % nvec16 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0;
  const int64_t nv = vec ? n / nvec16 : n;
  // at most ~2048 blocks: 32 chunks per sample, the rest over the batch
  const int64_t gx = std::min<int64_t>((nv + kThreads - 1) / kThreads, 32);
  const int64_t gy = std::min<int64_t>(B, std::max<int64_t>(1, 2048 / gx));
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto ttag, auto ctag, auto vtag) {
    using T = decltype(ttag);
    hipLaunchKernelGGL((batch_mix_kernel<T, decltype(ctag)::value, decltype(vtag)::value>), dim3(gx, gy),
                       dim3(kThreads), 0, stream, reinterpret_cast<const T*>(x.data_ptr()),
                       perm.data_ptr<int64_t>(), reinterpret_cast<T*>(out.data_ptr()), (int)B, (int)n, (int)C,
                       (int)W, (float)lam, (float)(1.0 - lam), mb);
  };
  auto by_mode = [&](auto ttag) {
    if (cut && vec) launch(ttag, std::true_type{}, std::true_type{});
    else if (cut) launch(ttag, std::true_type{}, std::false_type{});
    else if (vec) launch(ttag, std::false_type{}, std::true_type{});
    else launch(ttag, std::false_type{}, std::false_type{});
  };
  if (x.scalar_type() == at::kFloat) by_mode(float{});
  else by_mode(__bf16{});
  DMP_HIP_CHECK(hipGetLastError());
  return out;
}

}  // namespace dmp
