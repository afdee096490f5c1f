// Linear-layer side passes for the ViT MLP / attention projections on gfx950:
// the bias gradient (column sum of dy over all tokens) and the GELU backward
// fused with it.
//
// Why (profiles/vit_b16_bs128_1gpu_v3.md): PyTorch-ROCm computes each
// nn.Linear bias gradient with a generic reduce kernel (52 calls, 1.77 ms per
// ViT-B/16 step, ~2.4 TB/s) and the GELU backward as a separate elementwise
// pass (12 calls, 1.04 ms) whose output the fc1 bias reduce then reads again.
// Here:
//   * colsum: dy [M, N] bf16 -> per-block fp32 partial rows -> one column
//     reduce launch; every wave streams whole rows with 8-row unrolled loads
//     in flight;
//   * gelu_bwd_colsum: dh = dy * gelu'(h) (exact erf GELU, as nn.GELU()) written
//     once, and its column sums (fc1's bias gradient) taken from registers;
//   * rowscale_colsum: g = dy * s[sample of the row] written once, and its
//     column sums (stochastic depth: the gradient entering a scaled branch).
// Block = 4 waves; blockIdx.x picks a window of 64*VW columns (lane -> VW
// consecutive columns), blockIdx.y a chunk of rows; the 4 waves interleave
// rows and fold through LDS into one partial row per block.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "../colreduce.h"
#include "../api.h"
#include "../common.h"

namespace dmp {
namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 8;

template <int VW> struct BVec;  // VW bf16 values <-> f32
template <> struct BVec<8> {
  using raw = bf16x8;
};
template <> struct BVec<4> {
  using raw = bf16x4;
};

template <int VW>
__device__ __forceinline__ void to_f32(const typename BVec<VW>::raw& r, float (&v)[VW]) {
#pragma unroll
  for (int i = 0; i < VW; ++i) v[i] = (float)r[i];
}

__device__ __forceinline__ float gelu_grad(float h) {
  // d/dh [0.5 h (1 + erf(h / sqrt2))] = 0.5 (1 + erf(h / sqrt2)) + h * phi(h)
  constexpr float kInvSqrt2 = 0.70710678118654752f, kInvSqrt2Pi = 0.39894228040143268f;
  return 0.5f * (1.f + erff(h * kInvSqrt2)) + h * kInvSqrt2Pi * __expf(-0.5f * h * h);
}

template <int VW, bool GELU>
__global__ __launch_bounds__(kThreads) void colsum_kernel(const __bf16* __restrict__ dy,
                                                          const __bf16* __restrict__ h,
                                                          __bf16* __restrict__ dh, int64_t M,
                                                          int N, int rows_per_block,
                                                          float* __restrict__ part) {
  using raw = typename BVec<VW>::raw;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + lane) * VW;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  float acc[VW];
#pragma unroll
  for (int i = 0; i < VW; ++i) acc[i] = 0.f;
  if (col < N) {
    int64_t r = r0 + wid;
    for (; r + 4 * (kUnroll - 1) < r1; r += 4 * kUnroll) {
      raw a[kUnroll], b[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        a[u] = *reinterpret_cast<const raw*>(dy + (r + 4 * u) * N + col);
        if (GELU) b[u] = *reinterpret_cast<const raw*>(h + (r + 4 * u) * N + col);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        float g[VW];
        to_f32<VW>(a[u], g);
        if (GELU) {
          float hv[VW];
          to_f32<VW>(b[u], hv);
          raw o;
#pragma unroll
          for (int i = 0; i < VW; ++i) {
            g[i] *= gelu_grad(hv[i]);
            o[i] = (__bf16)g[i];
            g[i] = (float)o[i];  // sum what was stored: db == dh.sum(0) exactly
          }
          *reinterpret_cast<raw*>(dh + (r + 4 * u) * N + col) = o;
        }
#pragma unroll
        for (int i = 0; i < VW; ++i) acc[i] += g[i];
      }
    }
    for (; r < r1; r += 4) {
      float g[VW];
      to_f32<VW>(*reinterpret_cast<const raw*>(dy + r * N + col), g);
      if (GELU) {
        float hv[VW];
        to_f32<VW>(*reinterpret_cast<const raw*>(h + r * N + col), hv);
        raw o;
#pragma unroll
        for (int i = 0; i < VW; ++i) {
          g[i] *= gelu_grad(hv[i]);
          o[i] = (__bf16)g[i];
          g[i] = (float)o[i];
        }
        *reinterpret_cast<raw*>(dh + r * N + col) = o;
      }
#pragma unroll
      for (int i = 0; i < VW; ++i) acc[i] += g[i];
    }
  }
  __shared__ float red[kThreads / 64][64 * VW];
#pragma unroll
  for (int i = 0; i < VW; ++i) red[wid][lane * VW + i] = acc[i];
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * VW; e += kThreads) {
    const int c = blockIdx.x * 64 * VW + e;
    if (c < N) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < kThreads / 64; ++q) s += red[q][e];
      part[(int64_t)blockIdx.y * N + c] = s;
    }
  }
}

// Third variant (a sibling, so the two above keep their code): g = bf16(dy *
// s[row / rows_per_sample]) written once, and the column sums of the stored g
// -- the backward side pass of a residual branch scaled per sample
// (stochastic depth, ops/linear.py).  Same grid, unroll and fold.
template <int VW>
__global__ __launch_bounds__(kThreads) void rowscale_colsum_kernel(const __bf16* __restrict__ dy,
                                                                   const float* __restrict__ scale,
                                                                   unsigned rows_per_sample,
                                                                   __bf16* __restrict__ g, int64_t M, int N,
                                                                   int rows_per_block,
                                                                   float* __restrict__ part) {
  using raw = typename BVec<VW>::raw;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + lane) * VW;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  // row / rows_per_sample without a divide per row (M < 2^31, checked by the
  // host): hi32(row * floor((2^32 - 1) / d)) is the quotient or one below it
  const unsigned mg = 0xffffffffu / rows_per_sample;
  auto sample = [&](int64_t row) {
    const unsigned rw = (unsigned)row;
    const unsigned q = __umulhi(rw, mg);
    return q + (rw - q * rows_per_sample >= rows_per_sample ? 1u : 0u);
  };
  float acc[VW];
#pragma unroll
  for (int i = 0; i < VW; ++i) acc[i] = 0.f;
  if (col < N) {
    int64_t r = r0 + wid;
    for (; r + 4 * (kUnroll - 1) < r1; r += 4 * kUnroll) {
      raw a[kUnroll];
      float s[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        a[u] = *reinterpret_cast<const raw*>(dy + (r + 4 * u) * N + col);
        s[u] = scale[sample(r + 4 * u)];
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        float v[VW];
        to_f32<VW>(a[u], v);
        raw o;
#pragma unroll
        for (int i = 0; i < VW; ++i) {
          o[i] = (__bf16)(v[i] * s[u]);
          acc[i] += (float)o[i];  // sum what was stored: db == g.sum(0) exactly
        }
        *reinterpret_cast<raw*>(g + (r + 4 * u) * N + col) = o;
      }
    }
    for (; r < r1; r += 4) {
      float v[VW];
      to_f32<VW>(*reinterpret_cast<const raw*>(dy + r * N + col), v);
      const float s = scale[sample(r)];
      raw o;
#pragma unroll
      for (int i = 0; i < VW; ++i) {
        o[i] = (__bf16)(v[i] * s);
        acc[i] += (float)o[i];
      }
      *reinterpret_cast<raw*>(g + r * N + col) = o;
    }
  }
  __shared__ float red[kThreads / 64][64 * VW];
#pragma unroll
  for (int i = 0; i < VW; ++i) red[wid][lane * VW + i] = acc[i];
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * VW; e += kThreads) {
    const int c = blockIdx.x * 64 * VW + e;
    if (c < N) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < kThreads / 64; ++q) s += red[q][e];
      part[(int64_t)blockIdx.y * N + c] = s;
    }
  }
}

// rs: the third variant's per-sample scales and rows per sample (dh = its g)
struct RowScale {
  const float* scale;
  unsigned rows_per_sample;
};

void launch_colsum(const at::Tensor& dy, const at::Tensor* h, at::Tensor* dh, at::Tensor& db,
                   const RowScale* rs = nullptr) {
  const int64_t N = dy.size(-1), M = dy.numel() / N;
  const int VW = N % 512 == 0 ? 8 : 4;
  const int windows = (int)((N + 64 * VW - 1) / (64 * VW));
  // <= 256 row chunks (partial rows) per window, ~1024 blocks in total, at
  // least 4*kUnroll rows per block
  int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(256, 1024 / windows), M / (4 * kUnroll)));
  const int rows_per_block = (int)((M + chunks - 1) / chunks);
  chunks = (int)((M + rows_per_block - 1) / rows_per_block);
  auto part = at::empty({chunks, N}, dy.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid(windows, chunks);
  const __bf16* dyp = reinterpret_cast<const __bf16*>(dy.data_ptr());
  const __bf16* hp = h ? reinterpret_cast<const __bf16*>(h->data_ptr()) : nullptr;
  __bf16* dhp = dh ? reinterpret_cast<__bf16*>(dh->data_ptr()) : nullptr;
  if (M > 0 && rs) {
    if (VW == 8) hipLaunchKernelGGL((rowscale_colsum_kernel<8>), grid, dim3(kThreads), 0, stream, dyp, rs->scale, rs->rows_per_sample, dhp, M, (int)N, rows_per_block, part.data_ptr<float>());
    else hipLaunchKernelGGL((rowscale_colsum_kernel<4>), grid, dim3(kThreads), 0, stream, dyp, rs->scale, rs->rows_per_sample, dhp, M, (int)N, rows_per_block, part.data_ptr<float>());
  } else if (M > 0) {
    if (VW == 8) {
      if (h) hipLaunchKernelGGL((colsum_kernel<8, true>), grid, dim3(kThreads), 0, stream, dyp, hp, dhp, M, (int)N, rows_per_block, part.data_ptr<float>());
      else hipLaunchKernelGGL((colsum_kernel<8, false>), grid, dim3(kThreads), 0, stream, dyp, hp, dhp, M, (int)N, rows_per_block, part.data_ptr<float>());
    } else {
      if (h) hipLaunchKernelGGL((colsum_kernel<4, true>), grid, dim3(kThreads), 0, stream, dyp, hp, dhp, M, (int)N, rows_per_block, part.data_ptr<float>());
      else hipLaunchKernelGGL((colsum_kernel<4, false>), grid, dim3(kThreads), 0, stream, dyp, hp, dhp, M, (int)N, rows_per_block, part.data_ptr<float>());
    }
  } else {
    part.zero_();
  }
  const int n = (int)N;
  if (db.scalar_type() == at::kBFloat16)
    colreduce::launch(part.data_ptr<float>(), chunks, n, reinterpret_cast<__bf16*>(db.data_ptr()), stream);
  else
    colreduce::launch(part.data_ptr<float>(), chunks, n, db.data_ptr<float>(), stream);
}

void check_2d(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kBFloat16, name,
              " must be a contiguous bf16 GPU tensor");
  TORCH_CHECK(t.dim() >= 1 && t.size(-1) > 0 && t.size(-1) % 64 == 0, name, ": last dim must be a multiple of 64");
}

}  // namespace

bool colsum_supported(int64_t N) { return N > 0 && N % 64 == 0; }

// Bias gradient: dy [..., N] bf16 -> sum over all leading dims, in out_dtype.
at::Tensor bias_grad(const at::Tensor& dy, at::ScalarType out_dtype) {
  check_2d(dy, "dy");
  auto db = at::empty({dy.size(-1)}, dy.options().dtype(out_dtype));
  launch_colsum(dy, nullptr, nullptr, db);
  return db;
}

// fc1 backward through GELU: returns (dh = dy * gelu'(h), db = dh.sum(leading dims)).
std::vector<at::Tensor> gelu_bwd_bias_grad(const at::Tensor& dy, const at::Tensor& h,
                                           at::ScalarType out_dtype) {
  check_2d(dy, "dy");
  check_2d(h, "h");
  TORCH_CHECK(dy.sizes() == h.sizes(), "dy / h shape mismatch");
  auto dh = at::empty_like(h);
  auto db = at::empty({dy.size(-1)}, dy.options().dtype(out_dtype));
  launch_colsum(dy, &h, &dh, db);
  return {dh, db};
}

// Backward side pass of a residual branch scaled per sample (stochastic
// depth): returns (g = bf16(dy * row_scale[row / rows_per_sample]), db =
// g.sum(leading dims)) from one read of dy.
std::vector<at::Tensor> rowscale_bias_grad(const at::Tensor& dy, const at::Tensor& row_scale, int64_t rows_per_sample,
                                           at::ScalarType out_dtype) {
  check_2d(dy, "dy");
  const int64_t N = dy.size(-1), M = dy.numel() / N;
  TORCH_CHECK(row_scale.is_cuda() && row_scale.device() == dy.device() && row_scale.scalar_type() == at::kFloat &&
                  row_scale.is_contiguous(), "row_scale must be a contiguous fp32 tensor on dy's device");
  TORCH_CHECK(rows_per_sample > 0 && M < (1LL << 31), "rowscale_bias_grad: rows_per_sample > 0, rows < 2^31");
  TORCH_CHECK(row_scale.numel() * rows_per_sample == M, "rowscale_bias_grad: rows (", M,
              ") must be row_scale.numel() (", row_scale.numel(), ") * rows_per_sample (", rows_per_sample, ")");
  auto g = at::empty_like(dy);
  auto db = at::empty({N}, dy.options().dtype(out_dtype));
  const RowScale rs{row_scale.data_ptr<float>(), (unsigned)rows_per_sample};
  launch_colsum(dy, nullptr, &g, db, &rs);
  return {g, db};
}

}  // namespace dmp
