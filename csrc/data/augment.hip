// GPU-side image augmentation: random crop (zero padding or bilinear resize),
// horizontal flip, /255, mean / std normalisation, the cast to bf16 / fp32 and
// the output layout (channels-last or NCHW) of a uint8 NHWC batch in one launch.
//
// plan[i] = (x0, y0, cw, ch, flip) is sample i's crop box in source pixel
// coordinates (it may reach outside the image) and its flip bit.  For output
// pixel (dy, dx), dx' = flip ? out_w - 1 - dx : dx:
//   * cw == out_w and ch == out_h: the source pixel (y0 + dy, x0 + dx'), no
//     interpolation;
//   * otherwise the bilinear sample of F.interpolate(align_corners=False,
//     antialias=False) over the crop: sx = max(0, (dx' + 0.5) * cw / out_w - 0.5),
//     xl = floor(sx), xh = min(xl + 1, cw - 1), lx = sx - xl (same in y); the
//     taps clamp at the crop box and blend in fp32 in pixel units.
// A tap outside [0, Hs) x [0, Ws) reads as 0 (zero padding before the
// normalisation), so no plan makes the kernel read out of bounds.  A row with
// cw < 1 or ch < 1 reads nothing and writes its sample as NaN.
//
// Normalisation.  The no-resize path looks the byte up in a per-channel
// 256-entry table that the host builds with the very fp32 tensor ops of
// transforms.ToTensor + Normalize (staged in LDS, C * 256 floats), so it equals
// them bit for bit and divides nothing.  The resize path maps the blended
// value with one multiply-add per element (scale = 1 / (255 std), bias = -mean / std).
//
// The plan lives on the device and is never read back, so the host cannot see
// which path a row takes: the two paths are separate device functions and each
// block takes one of them per sample (block-uniform).  A caller that drew the
// plan and knows that no row resizes (pad-and-crop training, evaluation) says so
// (`no_resize`): that instantiation holds no interpolation code and needs half
// the registers; a row that resizes all the same is written as NaN, like a
// degenerate one.  Source coordinates go through
// fp64 ((dx' + 0.5) * cw / out_w - 0.5 as the fp64 reference forms it), once per
// output row / column of a lane, not per channel.
//
// A sample is one dense run of n = out_h * out_w * C output elements.  When n
// is a multiple of the 16-byte vector each lane produces one 16-byte store (8
// bf16 or 4 fp32; the output is freshly allocated, so every sample base is
// aligned), otherwise the scalar instantiation runs.  With C = 3 a
// channels-last vector straddles pixels: a lane decodes (y, x, c) of its first
// element once and walks the rest with carries (c -> x -> y; NCHW: x -> y -> c).
// The source is read by byte gathers (its alignment does not matter).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cmath>
#include <mutex>
#include "../api.h"
#include "../common.h"

namespace dmp {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxC = 4;

struct AugNorm {
  float scale[kMaxC], bias[kMaxC];
};

// a[c] of a kernel argument by two selects on c's bits (an equality chain the
// compiler turns into an indexed copy in scratch).
__device__ __forceinline__ float pick(const float (&a)[kMaxC], int c) {
  const float lo = (c & 1) ? a[1] : a[0], hi = (c & 1) ? a[3] : a[2];
  return (c & 2) ? hi : lo;
}

template <typename T, int N>
__device__ __forceinline__ void store_run(T* p, const float (&r)[N]) {
  if constexpr (N == 1) *p = (T)r[0];
  else Vec16<T>::store(p, r);
}

// (y, x, c) of output element e of a sample, and the step to element e + 1.
template <bool CL>
__device__ __forceinline__ void decode(int e, int C, int H, int W, int& y, int& x, int& c) {
  if constexpr (CL) {
    const unsigned pix = (unsigned)e / (unsigned)C;
    c = e - (int)pix * C;
    y = (int)(pix / (unsigned)W);
    x = (int)pix - y * W;
  } else {
    const unsigned row = (unsigned)e / (unsigned)W;
    x = e - (int)row * W;
    c = (int)(row / (unsigned)H);
    y = (int)row - c * H;
  }
}

template <bool CL>
__device__ __forceinline__ void advance(int C, int H, int W, int& y, int& x, int& c, bool& newx, bool& newy) {
  newx = newy = false;
  if constexpr (CL) {
    if (++c == C) {
      c = 0;
      newx = true;
      if (++x == W) {
        x = 0;
        ++y;
        newy = true;
      }
    }
  } else {
    newx = true;
    if (++x == W) {
      x = 0;
      newy = true;
      if (++y == H) {
        y = 0;
        ++c;
      }
    }
  }
}

// Box of the output's size: a copy through the table.  Coordinates are formed
// in unsigned arithmetic (no overflow for any int32 plan) and compared against
// the image, so an index is in bounds whenever it is used.
template <typename T, bool CL, int N>
__device__ __forceinline__ void crop_sample(const uint8_t* __restrict__ s, T* __restrict__ o, const float* tab, int x0,
                                            int y0, bool flip, int Hs, int Ws, int C, int H, int W, int nv, int step) {
  for (int v = blockIdx.x * kThreads + threadIdx.x; v < nv; v += step) {
    int y, x, c;
    decode<CL>(v * N, C, H, W, y, x, c);
    bool newx = true, newy = true;
    int row = -1, col = -1;  // source row offset (in pixels) / column, -1: outside the image
    float r[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (newy) {
        const unsigned sy = (unsigned)y0 + (unsigned)y;
        row = sy < (unsigned)Hs ? (int)sy * Ws : -1;
      }
      if (newx) {
        const unsigned sx = (unsigned)x0 + (unsigned)(flip ? W - 1 - x : x);
        col = sx < (unsigned)Ws ? (int)sx : -1;
      }
      // always an in-bounds load (offset c of the sample's first pixel when outside), zeroed after:
      // no branch around the gather, so the loads of a lane's elements are in flight together
      const bool in = row >= 0 && col >= 0;
      const int b = s[(in ? (row + col) * C : 0) + c];
      r[k] = tab[c * 256 + (in ? b : 0)];
      advance<CL>(C, H, W, y, x, c, newx, newy);
    }
    store_run<T, N>(o + (int64_t)v * N, r);
  }
}

// One axis of the bilinear sample: the two taps' source coordinates (or -1
// outside the image) and the weight of the second.
__device__ __forceinline__ void taps(int d, double f, int origin, int box, int limit, int& lo, int& hi, float& w) {
  const double sc = fmax(0.0, ((double)d + 0.5) * f - 0.5);
  const int l = (int)sc;  // < box
  const int h = min(l + 1, box - 1);
  w = (float)(sc - (double)l);
  const unsigned a = (unsigned)origin + (unsigned)l, b = (unsigned)origin + (unsigned)h;
  lo = a < (unsigned)limit ? (int)a : -1;
  hi = b < (unsigned)limit ? (int)b : -1;
}

template <typename T, bool CL, int N>
__device__ __forceinline__ void resize_sample(const uint8_t* __restrict__ s, T* __restrict__ o, const AugNorm& nrm,
                                              int x0, int y0, int cw, int ch, bool flip, int Hs, int Ws, int C, int H,
                                              int W, int nv, int step) {
  const double fx = (double)cw / (double)W, fy = (double)ch / (double)H;
  for (int v = blockIdx.x * kThreads + threadIdx.x; v < nv; v += step) {
    int y, x, c;
    decode<CL>(v * N, C, H, W, y, x, c);
    bool newx = true, newy = true;
    int r0 = -1, r1 = -1, c0 = -1, c1 = -1;  // tap rows (pixel offsets) / columns, -1: outside
    float ly = 0.f, lx = 0.f;
    float r[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (newy) {
        taps(y, fy, y0, ch, Hs, r0, r1, ly);
        r0 = r0 >= 0 ? r0 * Ws : -1;
        r1 = r1 >= 0 ? r1 * Ws : -1;
      }
      if (newx) taps(flip ? W - 1 - x : x, fx, x0, cw, Ws, c0, c1, lx);
      auto tap = [&](int row, int col) -> float {  // in bounds always, zeroed after (see crop_sample)
        const bool in = row >= 0 && col >= 0;
        const float b = (float)s[(in ? (row + col) * C : 0) + c];
        return in ? b : 0.f;
      };
      const float top = (1.f - lx) * tap(r0, c0) + lx * tap(r0, c1);
      const float bot = (1.f - lx) * tap(r1, c0) + lx * tap(r1, c1);
      const float val = (1.f - ly) * top + ly * bot;
      r[k] = val * pick(nrm.scale, c) + pick(nrm.bias, c);
      advance<CL>(C, H, W, y, x, c, newx, newy);
    }
    store_run<T, N>(o + (int64_t)v * N, r);
  }
}

// grid: x = chunks of one sample (grid-stride over its vectors), y = samples
// (grid-stride over the batch).  Hs * Ws * C and n are below 2^31 (host
// check), so indices within a sample are 32-bit; sample bases are 64-bit.
template <typename T, bool CL, bool RESIZE, bool VEC>
__global__ __launch_bounds__(kThreads) void augment_kernel(const uint8_t* __restrict__ src,
                                                           const int* __restrict__ plan, T* __restrict__ out,
                                                           const float* __restrict__ table, AugNorm nrm, int B, int Hs,
                                                           int Ws, int C, int H, int W) {
  constexpr int N = VEC ? Vec16<T>::N : 1;
  __shared__ float tab[kMaxC * 256];
  for (int i = threadIdx.x; i < C * 256; i += kThreads) tab[i] = table[i];
  __syncthreads();
  const int n = H * W * C;
  const int nv = n / N;  // VEC: n % N == 0
  const int step = gridDim.x * kThreads;
  const int64_t ns = (int64_t)Hs * Ws * C;
  for (int i = blockIdx.y; i < B; i += gridDim.y) {
    const int* p = plan + (int64_t)i * 5;
    const int x0 = p[0], y0 = p[1], cw = p[2], ch = p[3];
    const bool flip = p[4] != 0;
    const uint8_t* s = src + (int64_t)i * ns;
    T* o = out + (int64_t)i * n;
    const bool same = cw == W && ch == H;
    if (cw < 1 || ch < 1 || (!RESIZE && !same)) {  // block-uniform: degenerate (or unannounced) box, nothing read
      float r[N];
#pragma unroll
      for (int k = 0; k < N; ++k) r[k] = __builtin_nanf("");
      for (int v = blockIdx.x * kThreads + threadIdx.x; v < nv; v += step) store_run<T, N>(o + (int64_t)v * N, r);
    } else if (same) {
      crop_sample<T, CL, N>(s, o, tab, x0, y0, flip, Hs, Ws, C, H, W, nv, step);
    } else if constexpr (RESIZE) {
      resize_sample<T, CL, N>(s, o, nrm, x0, y0, cw, ch, flip, Hs, Ws, C, H, W, nv, step);
    }
  }
}

// The table of the no-resize path, [C, 256] fp32 on `dev`: entry (c, v) is
// Normalize(mean, std)(ToTensor(v)) formed with the same fp32 tensor ops as
// data/transforms.py.  Built once per (device, mean, std) and kept (until the
// process ends), so a step copies nothing to the device.  The first call for a
// (device, mean, std) does copy: a blocking pageable host-to-device copy, which
// a stream capture would refuse -- make one call before capturing.
at::Tensor norm_table(const std::vector<double>& mean, const std::vector<double>& std_, const at::Device& dev) {
  struct Entry {
    int dev;
    std::vector<double> mean, std_;
    at::Tensor table;
  };
  static std::mutex mu;
  static std::vector<Entry> cache;
  std::lock_guard<std::mutex> lock(mu);
  for (const Entry& e : cache)
    if (e.dev == dev.index() && e.mean == mean && e.std_ == std_) return e.table;
  const int64_t C = (int64_t)mean.size();
  auto t = at::arange(256, at::TensorOptions().dtype(at::kByte)).to(at::kFloat).div_(255.0).view({1, 256});
  auto m = at::tensor(at::ArrayRef<double>(mean), at::TensorOptions().dtype(at::kDouble)).to(at::kFloat).view({C, 1});
  auto s = at::tensor(at::ArrayRef<double>(std_), at::TensorOptions().dtype(at::kDouble)).to(at::kFloat).view({C, 1});
  auto table = ((t - m) / s).contiguous().to(dev);
  if (cache.size() >= 16) cache.clear();
  cache.push_back(Entry{(int)dev.index(), mean, std_, table});
  return table;
}

}  // namespace

// src: dense uint8 [B, Hs, Ws, C] on the GPU; plan: int32 [B, 5] rows (x0, y0, cw, ch, flip)
// on src's device; out: new [B, C, out_h, out_w] bf16 / fp32, dense channels-last or NCHW.
// no_resize: the caller's word that every row has cw == out_w and ch == out_h (others come out NaN).
at::Tensor augment_batch(const at::Tensor& src, const at::Tensor& plan, int64_t out_h, int64_t out_w,
                         const std::vector<double>& mean, const std::vector<double>& std_, at::ScalarType dtype,
                         bool channels_last, bool no_resize) {
  TORCH_CHECK(src.is_cuda() && src.dim() == 4 && src.scalar_type() == at::kByte && src.is_contiguous(),
              "augment_batch: src must be a dense uint8 [B, Hs, Ws, C] GPU tensor");
  const int64_t B = src.size(0), Hs = src.size(1), Ws = src.size(2), C = src.size(3);
  TORCH_CHECK(C >= 1 && C <= kMaxC, "augment_batch: C must be in [1, ", kMaxC, "], got ", C);
  TORCH_CHECK(plan.is_cuda() && plan.device() == src.device() && plan.scalar_type() == at::kInt && plan.dim() == 2 &&
                  plan.size(0) == B && plan.size(1) == 5 && plan.is_contiguous(),
              "augment_batch: plan must be a contiguous int32 [B, 5] tensor on src's device");
  TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16, "augment_batch: dtype must be fp32 or bf16");
  TORCH_CHECK((int64_t)mean.size() == C && (int64_t)std_.size() == C, "augment_batch: mean and std need C = ", C,
              " entries");
  for (double s : std_) TORCH_CHECK(s != 0.0 && std::isfinite(s), "augment_batch: std entries must be non-zero");
  for (int64_t v : {Hs, Ws, out_h, out_w})
    TORCH_CHECK(v >= 1 && v <= 16384, "augment_batch: image sides must be in [1, 16384], got ", v);
  const int64_t n = out_h * out_w * C;
  TORCH_CHECK(Hs * Ws * C < (int64_t(1) << 31) && n < (int64_t(1) << 31) && B < (int64_t(1) << 31),
              "augment_batch: sample or batch too large");
  auto opts = src.options().dtype(dtype);
  auto out = at::empty({B, C, out_h, out_w}, opts,
                       channels_last ? at::MemoryFormat::ChannelsLast : at::MemoryFormat::Contiguous);
  if (B == 0) return out;
  const at::Tensor table = norm_table(mean, std_, src.device());
  AugNorm nrm{};
  for (int64_t c = 0; c < C; ++c) {  // from the fp32 mean / std the table uses
    const double m = (double)(float)mean[c], s = (double)(float)std_[c];
    nrm.scale[c] = (float)(1.0 / (255.0 * s));
    nrm.bias[c] = (float)(-m / s);
  }
  const int64_t nvec16 = 16 / out.element_size();
  const bool vec = n % nvec16 == 0 && reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0;
  const int64_t nv = vec ? n / nvec16 : n;
  // at most ~2048 blocks: 32 chunks per sample, the rest over the batch
  const int64_t gx = std::min<int64_t>((nv + kThreads - 1) / kThreads, 32);
  const int64_t gy = std::min<int64_t>(B, std::max<int64_t>(1, 2048 / gx));
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto ttag, auto ltag, auto rtag, auto vtag) {
    using T = decltype(ttag);
    hipLaunchKernelGGL((augment_kernel<T, decltype(ltag)::value, decltype(rtag)::value, decltype(vtag)::value>),
                       dim3(gx, gy),
                       dim3(kThreads), 0, stream, src.data_ptr<uint8_t>(), plan.data_ptr<int>(),
                       reinterpret_cast<T*>(out.data_ptr()), table.data_ptr<float>(), nrm, (int)B, (int)Hs, (int)Ws,
                       (int)C, (int)out_h, (int)out_w);
  };
  auto by_layout = [&](auto ttag, auto rtag) {
    if (channels_last && vec) launch(ttag, std::true_type{}, rtag, std::true_type{});
    else if (channels_last) launch(ttag, std::true_type{}, rtag, std::false_type{});
    else if (vec) launch(ttag, std::false_type{}, rtag, std::true_type{});
    else launch(ttag, std::false_type{}, rtag, std::false_type{});
  };
  auto by_path = [&](auto ttag) {
    if (no_resize) by_layout(ttag, std::false_type{});
    else by_layout(ttag, std::true_type{});
  };
  if (dtype == at::kFloat) by_path(float{});
  else by_path(__bf16{});
  DMP_HIP_CHECK(hipGetLastError());
  return out;
}

}  // namespace dmp
