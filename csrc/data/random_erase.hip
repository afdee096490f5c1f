// Random erasing (timm's RandomErasing, count = 1) on the normalised batch
// x [B, C, H, W], bf16 or fp32, dense channels-last or NCHW, 1 <= C <= 4, in
// place, one launch.  boxes[b] = (x0, y0, w, h, k0, k1): sample b's box in
// image pixel coordinates (w == 0: not erased) and the two words of its 64-bit
// key.  The host draws and checks the plan (data/random_erase.py), so no box
// leaves the image; all the same a lane whose pixel is outside the image
// writes nothing.
//
// Inside the box, channel c of pixel (y, x), absolute image coordinates:
//   noise:  (r0, r1, r2, r3) = Philox4x32-10(counter (x, y, 0, 0), key (k0, k1)) (philox.h),
//           u_i = (2 (r_i >> 9) + 1) 2^-24, Box-Muller in fp32 with the precise logf /
//           sqrtf / sincospif:  z0 = sqrt(-2 ln u0) cos(2 pi u1), z1 = ... sin(2 pi u1),
//           z2, z3 likewise from u2, u3;  x[b, c, y, x] = z_c, rounded once to the dtype
//   else:   x[b, c, y, x] = fill[b, c] (0 without fill)
// The noise is a function of (key, x, y, c) alone: layout, dtype, the box's
// position in the grid and the sample's place in the batch do not enter.
//
// Kernels of this file: random_erase_kernel<T, CL> for T in {float, bf16} and
// CL in {channels-last, NCHW} = 4, and philox_bits_kernel = 5 kernels.
// No LDS, no atomics, no scratch.
//
// grid = (tiles(max w), tiles(max h), B) with 64 x 4 pixel tiles, the maxima
// taken from the host plan; a block is 4 waves, each one 64-pixel row segment.
// A block whose sample is not erased or whose tile lies outside its box
// returns at once.  A lane owns one pixel: one Philox call, then the C stores.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "../api.h"
#include "../common.h"
#include "philox.h"

namespace dmp {
namespace {

constexpr int kTileW = 64;  // one wave
constexpr int kTileH = 4;
constexpr int kMaxC = 4;

__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& za, float& zb) {
  const float r = sqrtf(-2.f * logf(philox_uniform(ra)));
  float s, c;
  sincospif(2.f * philox_uniform(rb), &s, &c);  // 2 u is exact: the angle is never rounded
  za = r * c;
  zb = r * s;
}

template <typename T, bool CL>
__global__ __launch_bounds__(kTileW* kTileH) void random_erase_kernel(T* __restrict__ x,
                                                                      const int* __restrict__ boxes,
                                                                      const float* __restrict__ fill, bool noise,
                                                                      int C, int H, int W) {
  const int b = blockIdx.z;
  const int* p = boxes + (int64_t)b * 6;
  const int w = p[2], h = p[3];
  if (w <= 0 || h <= 0 || (int)blockIdx.x * kTileW >= w || (int)blockIdx.y * kTileH >= h) return;  // block-uniform
  const int px = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
  const int py = blockIdx.y * kTileH + (threadIdx.x / kTileW);
  if (px >= w || py >= h) return;
  const unsigned X = (unsigned)p[0] + (unsigned)px, Y = (unsigned)p[1] + (unsigned)py;
  if (X >= (unsigned)W || Y >= (unsigned)H) return;  // never for a checked plan
  float z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
  if (noise) {
    const Philox4 r = philox4x32_10(X, Y, 0u, 0u, (uint32_t)p[4], (uint32_t)p[5]);
    box_muller(r.v[0], r.v[1], z0, z1);
    if (C > 2) box_muller(r.v[2], r.v[3], z2, z3);
  } else if (fill != nullptr) {
    const float* f = fill + (int64_t)b * C;
    z0 = f[0];
    if (C > 1) z1 = f[1];
    if (C > 2) z2 = f[2];
    if (C > 3) z3 = f[3];
  }
  // element (b, c, Y, X): its offset for c = 0 and the step to the next channel
  const int64_t pix = (int64_t)Y * W + X;
  const int64_t base = CL ? ((int64_t)b * H * W + pix) * C : (int64_t)b * C * H * W + pix;
  const int64_t cs = CL ? 1 : (int64_t)H * W;
  x[base] = (T)z0;
  if (C > 1) x[base + cs] = (T)z1;
  if (C > 2) x[base + 2 * cs] = (T)z2;
  if (C > 3) x[base + 3 * cs] = (T)z3;
}

__global__ __launch_bounds__(256) void philox_bits_kernel(const int* __restrict__ counters,
                                                          const int* __restrict__ key, int* __restrict__ out,
                                                          int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int* c = counters + i * 4;
  const Philox4 r = philox4x32_10((uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2], (uint32_t)c[3], (uint32_t)key[0],
                                  (uint32_t)key[1]);
  int* o = out + i * 4;
  o[0] = (int)r.v[0];
  o[1] = (int)r.v[1];
  o[2] = (int)r.v[2];
  o[3] = (int)r.v[3];
}

}  // namespace

// x: dense channels-last or NCHW [B, C, H, W] bf16 / fp32 on the GPU, 1 <= C <= 4, written in place.
// boxes: host int32 [B, 6] rows (x0, y0, w, h, k0, k1); every row is checked here again (the kernel
// never sees a box that leaves the image) and the plan goes up non-blocking (pin it for that to hold).
// fill: none, or host float32 [B, C] (noise must then be false).  No erased row: nothing is launched.
void random_erase(const at::Tensor& x, const at::Tensor& boxes, const c10::optional<at::Tensor>& fill, bool noise) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "random_erase: x must be a 4-D GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16,
              "random_erase: x must be fp32 or bf16");
  const int64_t B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(C >= 1 && C <= kMaxC, "random_erase: C must be in [1, ", kMaxC, "], got ", C);
  const bool nchw = x.is_contiguous();
  TORCH_CHECK(nchw || x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "random_erase: x must be dense, channels-last or NCHW");
  TORCH_CHECK(H < (int64_t(1) << 31) && W < (int64_t(1) << 31) && B <= 65535,
              "random_erase: image side or batch too large (B <= 65535)");
  TORCH_CHECK(boxes.is_cpu() && boxes.scalar_type() == at::kInt && boxes.dim() == 2 && boxes.size(0) == B &&
                  boxes.size(1) == 6 && boxes.is_contiguous(),
              "random_erase: boxes must be a contiguous host int32 [B, 6] tensor");
  if (fill.has_value()) {
    TORCH_CHECK(!noise, "random_erase: fill and noise exclude each other");
    TORCH_CHECK(fill->is_cpu() && fill->scalar_type() == at::kFloat && fill->dim() == 2 && fill->size(0) == B &&
                    fill->size(1) == C && fill->is_contiguous(),
                "random_erase: fill must be a contiguous host float32 [B, C] tensor");
  }
  const int* p = boxes.data_ptr<int>();
  int64_t max_w = 0, max_h = 0;
  for (int64_t i = 0; i < B; ++i, p += 6) {
    const int64_t x0 = p[0], y0 = p[1], w = p[2], h = p[3];
    TORCH_CHECK(x0 >= 0 && y0 >= 0 && w >= 0 && h >= 0 && x0 + w <= W && y0 + h <= H && (w == 0) == (h == 0),
                "random_erase: boxes row ", i, " leaves the ", H, " x ", W, " image or is half empty");
    max_w = std::max(max_w, w);
    max_h = std::max(max_h, h);
  }
  if (max_w == 0) return;
  const at::Tensor dboxes = boxes.to(x.device(), /*non_blocking=*/true);
  at::Tensor dfill;
  if (fill.has_value()) dfill = fill->to(x.device(), /*non_blocking=*/true);
  const float* fp = fill.has_value() ? dfill.data_ptr<float>() : nullptr;
  const dim3 grid((unsigned)((max_w + kTileW - 1) / kTileW), (unsigned)((max_h + kTileH - 1) / kTileH), (unsigned)B);
  TORCH_CHECK(grid.y <= 65535, "random_erase: box too tall");
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto ttag, auto ltag) {
    using T = decltype(ttag);
    hipLaunchKernelGGL((random_erase_kernel<T, decltype(ltag)::value>), grid, dim3(kTileW * kTileH), 0, stream,
                       reinterpret_cast<T*>(x.data_ptr()), dboxes.data_ptr<int>(), fp, noise, (int)C, (int)H, (int)W);
  };
  auto by_layout = [&](auto ttag) {
    if (nchw) launch(ttag, std::false_type{});
    else launch(ttag, std::true_type{});
  };
  if (x.scalar_type() == at::kFloat) by_layout(float{});
  else by_layout(__bf16{});
  DMP_HIP_CHECK(hipGetLastError());
}

// counters: int32 [n, 4] and key: int32 [2] on one GPU (bit patterns of unsigned words);
// out[i] = Philox4x32-10(counters[i], key), the generator of philox.h as the device runs it.
at::Tensor philox_bits(const at::Tensor& counters, const at::Tensor& key) {
  TORCH_CHECK(counters.is_cuda() && counters.scalar_type() == at::kInt && counters.dim() == 2 &&
                  counters.size(1) == 4 && counters.is_contiguous(),
              "philox_bits: counters must be a contiguous int32 [n, 4] GPU tensor");
  TORCH_CHECK(key.is_cuda() && key.device() == counters.device() && key.scalar_type() == at::kInt &&
                  key.dim() == 1 && key.size(0) == 2 && key.is_contiguous(),
              "philox_bits: key must be a contiguous int32 [2] tensor on the counters' device");
  auto out = at::empty_like(counters);
  const int64_t n = counters.size(0);
  if (n == 0) return out;
  TORCH_CHECK(n < (int64_t(1) << 31), "philox_bits: too many counters");
  hipLaunchKernelGGL(philox_bits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     at::hip::getCurrentHIPStream(), counters.data_ptr<int>(), key.data_ptr<int>(),
                     out.data_ptr<int>(), n);
  DMP_HIP_CHECK(hipGetLastError());
  return out;
}

}  // namespace dmp
