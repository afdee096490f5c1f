// RandAugment on the GPU: the 15 "increasing" ops of rand-m9-mstd0.5-inc1 over a
// uint8 [B, H, W, 3] batch, byte in, byte out, rounding to bytes between ops as
// PIL does.  The definition of every op (and of the byte crop) is the docstring
// of data/rand_augment.py; its PyTorch composition is what these kernels equal
// bit for bit.  All randomness is drawn on the host: ops int32 [B, n] holds one
// op code per sample and slot (kNotApplied for a slot whose op was not
// applied), args float64 [B, n, 6] its argument (args[0]: bits, threshold,
// addend or blend factor; the affine ops: the six matrix coefficients).
//
// Launches for n slots: crop_bytes_kernel, then per slot rand_hist_kernel (only
// when the slot holds AutoContrast, Equalize or ContrastIncreasing somewhere in
// the batch) and rand_apply_kernel; the histograms of all slots are zeroed by
// one memset.  n = 2: 5 kernel launches.
//
//   crop_bytes_kernel   augment_batch's plan rows -> uint8 [B, H, W, 3]: a copy
//                       (zero outside the image), or the bilinear sample with
//                       fp64 tap coordinates and an fp32 blend of separately
//                       rounded operations, rint (half to even) of the clamp.
//   rand_hist_kernel    four 256-bin int32 histograms per sample (r, g, b, gray)
//                       in LDS, added to [B, 4, 256] with integer atomics: the
//                       counts are exact, so the order does not matter.  A
//                       sample fills the ones its op reads (ContrastIncreasing:
//                       gray; AutoContrast, Equalize: r, g, b); blocks of
//                       samples whose op needs none leave at once.
//   rand_apply_kernel   one pass per slot, path chosen per sample (block-uniform):
//                       a per-channel 256-byte table built in LDS by each block
//                       from (op, argument, histograms) -- min, max, gray mean
//                       and the Equalize prefix sums all come from the histograms
//                       -- or Color (per pixel), Sharpness (3 x 3 gather), affine
//                       (gather).  Slots before the last write uint8 into a
//                       staging buffer (ping-pong, never in place); the last one
//                       looks the byte up in the [3, 256] fp32 normalisation
//                       table (Normalize(ToTensor(v)), the table of augment.hip's
//                       no-resize path, built by the caller with those tensor
//                       ops) and writes bf16 / fp32, channels-last or NCHW, with
//                       16-byte stores when the sample size allows.
//
// Bounds.  Sharpness clamps its neighbour coordinates into the image; an affine
// source coordinate is compared against the image (a NaN fails the comparison)
// and replaced by the fill colour otherwise; the crop compares every tap as
// augment.hip does.  A sample with an op code outside the table or a non-finite
// argument in any slot reads nothing and comes out NaN.
//
// Exact arithmetic.  Every formula that must equal the elementwise PyTorch
// oracle sits in a __forceinline__ function under `#pragma clang fp
// contract(off)`: hipcc contracts a + f * (b - a) into a fused multiply-add
// otherwise (the __fmul_rn / __fadd_rn intrinsics do not stop it).
//
// LDS (kApplyLdsBytes): histograms 4 x 256 x 4 + byte tables 3 x 256 +
// normalisation table 3 x 256 x 4 = 7936 bytes (the staging instantiations hold
// no normalisation table); rand_hist_kernel: the histograms, 4096 bytes.  No
// scratch: every per-lane array is indexed by unrolled constants only.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cmath>
#include "../api.h"
#include "../common.h"

namespace dmp {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxSlots = 8;
constexpr int kArgs = 6;
constexpr int kHistInts = 4 * 256;
constexpr int kApplyLdsBytes = kHistInts * 4 + 3 * 256 + 3 * 256 * 4;
static_assert(kApplyLdsBytes == 7936, "keep the file comment and tests/test_rand_augment_resources.py in step");

// the op codes of data/rand_augment.py (OPS), in order
enum Op : int {
  kAutoContrast = 0, kEqualize, kInvert, kPosterize, kSolarize, kSolarizeAdd, kBrightness, kContrast,
  kColor, kSharpness, kShearX, kShearY, kTranslateX, kTranslateY, kRotate, kNotApplied, kNumCodes
};

struct Fill {
  int r, g, b;
};

__device__ __forceinline__ bool needs_hist(int op) { return op == kAutoContrast || op == kEqualize || op == kContrast; }

__device__ __forceinline__ int pick3(int c, int r, int g, int b) { return c == 0 ? r : (c == 1 ? g : b); }

__device__ __forceinline__ int gray_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// ---- the formulas that must round as the oracle's separate tensor ops do ----
__device__ __forceinline__ int blend(float d, float v, float f) {
#pragma clang fp contract(off)
  const float diff = v - d;
  const float prod = f * diff;
  const float t = d + prod;
  return (int)fminf(fmaxf(t, 0.f), 255.f);
}

__device__ __forceinline__ int autocontrast_entry(int v, int lo, int hi) {
#pragma clang fp contract(off)
  const double scale = 255.0 / (double)(hi - lo);
  const double off = -(double)lo * scale;
  const double prod = (double)v * scale;
  const double t = prod + off;
  return min(255, max(0, (int)t));
}

__device__ __forceinline__ int mean_level(long long sum, int count) {
#pragma clang fp contract(off)
  const double mean = (double)sum / (double)count;
  return (int)(mean + 0.5);
}

struct Mat {
  double a, b, c, d, e, g;
};

// source byte offset of output pixel (y, x) under the affine map, or -1: the fill colour
__device__ __forceinline__ int affine_source(const Mat& m, int y, int x, int H, int W) {
#pragma clang fp contract(off)
  const double px = (double)x + 0.5, py = (double)y + 0.5;
  const double ax = m.a * px, bx = m.b * py, ay = m.d * px, by = m.e * py;
  const double sx = ax + bx, sy = ay + by;
  const double xi = sx + m.c, yi = sy + m.g;
  const bool in = xi >= 0.0 && xi < (double)W && yi >= 0.0 && yi < (double)H;  // false for NaN
  return in ? ((int)yi * W + (int)xi) * 3 : -1;  // 0 <= (int)xi < W, 0 <= (int)yi < H
}

// One axis of the bilinear sample (the coordinates of augment.hip's taps(), each
// operation rounded on its own): the two taps' source coordinates (-1 outside
// the image) and the weight of the second.
__device__ __forceinline__ void byte_taps(int d, double f, int origin, int box, int limit, int& lo, int& hi, float& w) {
#pragma clang fp contract(off)
  const double prod = ((double)d + 0.5) * f;
  const double sc = fmax(0.0, prod - 0.5);
  const int l = min((int)sc, box - 1);
  const int h = min(l + 1, box - 1);
  w = (float)(sc - (double)l);
  const unsigned a = (unsigned)origin + (unsigned)l, b = (unsigned)origin + (unsigned)h;
  lo = a < (unsigned)limit ? (int)a : -1;
  hi = b < (unsigned)limit ? (int)b : -1;
}

__device__ __forceinline__ int bilerp_byte(float lx, float ly, float t00, float t01, float t10, float t11) {
#pragma clang fp contract(off)
  const float wx = 1.f - lx, wy = 1.f - ly;
  const float a0 = wx * t00, a1 = lx * t01, b0 = wx * t10, b1 = lx * t11;
  const float top = a0 + a1, bot = b0 + b1;
  const float c0 = wy * top, c1 = ly * bot;
  const float val = c0 + c1;
  return (int)rintf(fminf(fmaxf(val, 0.f), 255.f));
}

// ---- crop to bytes ----
// grid: x = chunks of one sample's pixels, y = samples (both grid-stride).  A
// row with cw < 1 or ch < 1 reads nothing and is written as zeros (bytes hold no
// NaN; data/rand_augment.py refuses such a plan before the launch).
__global__ __launch_bounds__(kThreads) void crop_bytes_kernel(const uint8_t* __restrict__ src,
                                                              const int* __restrict__ plan, uint8_t* __restrict__ out,
                                                              int B, int Hs, int Ws, int H, int W) {
  const int np = H * W;
  const int step = gridDim.x * kThreads;
  const int64_t ns = (int64_t)Hs * Ws * 3;
  for (int i = blockIdx.y; i < B; i += gridDim.y) {
    const int* p = plan + (int64_t)i * 5;
    const int x0 = p[0], y0 = p[1], cw = p[2], ch = p[3];
    const bool flip = p[4] != 0;
    const uint8_t* s = src + (int64_t)i * ns;
    uint8_t* o = out + (int64_t)i * np * 3;
    if (cw < 1 || ch < 1) {  // block-uniform
      for (int q = blockIdx.x * kThreads + threadIdx.x; q < np; q += step) o[q * 3] = o[q * 3 + 1] = o[q * 3 + 2] = 0;
    } else if (cw == W && ch == H) {
      for (int q = blockIdx.x * kThreads + threadIdx.x; q < np; q += step) {
        const int y = q / W, x = q - y * W;
        const unsigned sy = (unsigned)y0 + (unsigned)y, sx = (unsigned)x0 + (unsigned)(flip ? W - 1 - x : x);
        const bool in = sy < (unsigned)Hs && sx < (unsigned)Ws;
        const uint8_t* t = s + (in ? ((int)sy * Ws + (int)sx) * 3 : 0);  // always in bounds, zeroed after
        const int r = t[0], g = t[1], b = t[2];
        o[q * 3] = in ? r : 0;
        o[q * 3 + 1] = in ? g : 0;
        o[q * 3 + 2] = in ? b : 0;
      }
    } else {
      const double fx = (double)cw / (double)W, fy = (double)ch / (double)H;
      for (int q = blockIdx.x * kThreads + threadIdx.x; q < np; q += step) {
        const int y = q / W, x = q - y * W;
        int r0, r1, c0, c1;
        float ly, lx;
        byte_taps(y, fy, y0, ch, Hs, r0, r1, ly);
        byte_taps(flip ? W - 1 - x : x, fx, x0, cw, Ws, c0, c1, lx);
        auto tap = [&](int row, int col, int c) -> float {  // in bounds always, zeroed after
          const bool in = row >= 0 && col >= 0;
          const float b = (float)s[(in ? (row * Ws + col) * 3 : 0) + c];
          return in ? b : 0.f;
        };
#pragma unroll
        for (int c = 0; c < 3; ++c)
          o[q * 3 + c] = (uint8_t)bilerp_byte(lx, ly, tap(r0, c0, c), tap(r0, c1, c), tap(r1, c0, c), tap(r1, c1, c));
      }
    }
  }
}

// Every slot of sample i holds a known op code and finite arguments (the same
// answer in every lane and every block of the sample).
__device__ __forceinline__ bool sample_ok(const int* __restrict__ ops, const double* __restrict__ args, int i, int n) {
  bool ok = true;
  for (int s = 0; s < n; ++s) {
    const int64_t k = (int64_t)i * n + s;
    ok = ok && (unsigned)ops[k] < (unsigned)kNumCodes;
    for (int a = 0; a < kArgs; ++a) ok = ok && isfinite(args[k * kArgs + a]);
  }
  return ok;
}

// ---- histograms ----
// img: uint8 [B, np, 3]; hist: int32 [B, 4, 256] of this slot, zero on entry.
__global__ __launch_bounds__(kThreads) void rand_hist_kernel(const uint8_t* __restrict__ img,
                                                             const int* __restrict__ ops,
                                                             const double* __restrict__ args, int* __restrict__ hist,
                                                             int B, int n, int slot, int np) {
  __shared__ int h[kHistInts];
  const int step = gridDim.x * kThreads;
  for (int i = blockIdx.y; i < B; i += gridDim.y) {
    const int op = ops[(int64_t)i * n + slot];
    if (!sample_ok(ops, args, i, n) || !needs_hist(op)) continue;  // block-uniform
    for (int k = threadIdx.x; k < kHistInts; k += kThreads) h[k] = 0;
    __syncthreads();
    const uint8_t* s = img + (int64_t)i * np * 3;
    const bool gray_only = op == kContrast;  // the one op that reads the gray histogram reads no other
    for (int q = blockIdx.x * kThreads + threadIdx.x; q < np; q += step) {
      const int r = s[q * 3], g = s[q * 3 + 1], b = s[q * 3 + 2];
      if (gray_only) {
        atomicAdd(&h[768 + gray_of(r, g, b)], 1);  // gray_of <= 255: the weights sum to 65536
      } else {
        atomicAdd(&h[r], 1);
        atomicAdd(&h[256 + g], 1);
        atomicAdd(&h[512 + b], 1);
      }
    }
    __syncthreads();
    int* dst = hist + (int64_t)i * kHistInts;
    for (int k = threadIdx.x; k < kHistInts; k += kThreads)
      if (h[k] != 0) atomicAdd(&dst[k], h[k]);
    __syncthreads();
  }
}

// ---- apply ----
// (y, x, c) of element e of a sample (channels-last or NCHW, C = 3) and the step to e + 1.
template <bool CL>
__device__ __forceinline__ void decode3(int e, int H, int W, int& y, int& x, int& c) {
  if constexpr (CL) {
    const unsigned pix = (unsigned)e / 3u;
    c = e - (int)pix * 3;
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
__device__ __forceinline__ void advance3(int H, int W, int& y, int& x, int& c, bool& newpix) {
  if constexpr (CL) {
    newpix = false;
    if (++c == 3) {
      c = 0;
      newpix = true;
      if (++x == W) {
        x = 0;
        ++y;
      }
    }
  } else {
    newpix = true;
    if (++x == W) {
      x = 0;
      if (++y == H) {
        y = 0;
        ++c;
      }
    }
  }
}

// N consecutive output elements of a lane: the normalised values (last slot) or the bytes (staging).
template <typename T, int N, bool LAST>
struct Run {
  float r[LAST ? N : 1];
  uint32_t w[LAST ? 1 : (N + 3) / 4];
  __device__ __forceinline__ void clear() {
    if constexpr (!LAST) {
#pragma unroll
      for (int k = 0; k < (N + 3) / 4; ++k) w[k] = 0;
    }
  }
  __device__ __forceinline__ void put(int k, int byte, int c, const float* tab) {  // k: an unrolled constant
    if constexpr (LAST) r[k] = tab[c * 256 + byte];
    else w[k / 4] |= (uint32_t)byte << (8 * (k % 4));
  }
  __device__ __forceinline__ void store(T* p) const {
    if constexpr (LAST) {
      if constexpr (N == 1) *p = (T)r[0];
      else Vec16<T>::store(p, r);
    } else {
      if constexpr (N == 1) *p = (T)w[0];
      else {
        u32x4 q;
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = w[k];
        *reinterpret_cast<u32x4*>(p) = q;
      }
    }
  }
};

// The element loop of one sample: byte_at(y, x, c, newpix) gives the op's output byte.
template <typename T, bool CL, int N, bool LAST, typename F>
__device__ __forceinline__ void run_sample(T* __restrict__ o, const float* tab, int H, int W, int nv, int step,
                                           F&& byte_at) {
  for (int v = blockIdx.x * kThreads + threadIdx.x; v < nv; v += step) {
    int y, x, c;
    decode3<CL>(v * N, H, W, y, x, c);
    bool newpix = true;
    Run<T, N, LAST> run;
    run.clear();
#pragma unroll
    for (int k = 0; k < N; ++k) {
      run.put(k, byte_at(y, x, c, newpix), c, tab);
      advance3<CL>(H, W, y, x, c, newpix);
    }
    run.store(o + (int64_t)v * N);
  }
}

// Entry v = threadIdx.x of the three byte tables of a table op.  hs: the sample's histograms
// in LDS (read only by the ops that need them).  Out-of-range integer arguments are clamped.
__device__ __forceinline__ void build_tables(uint8_t* lut, const int* hs, int op, double a0, int np) {
  const int v = threadIdx.x;
  const double ai = fmin(fmax(a0, 0.0), 256.0);
  const float f = (float)a0;
  int level = 0;
  if (op == kContrast) {
    long long sum = 0;
    for (int j = 0; j < 256; ++j) sum += (long long)j * hs[768 + j];
    level = mean_level(sum, np);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int e = v;
    if (op == kAutoContrast) {
      int lo = 256, hi = -1;
      for (int j = 0; j < 256; ++j)
        if (hs[c * 256 + j] != 0) {
          lo = min(lo, j);
          hi = j;
        }
      if (hi > lo) e = autocontrast_entry(v, lo, hi);
    } else if (op == kEqualize) {
      int total = 0, nz = 0, last = 0, before = 0;
      for (int j = 0; j < 256; ++j) {
        const int hj = hs[c * 256 + j];
        total += hj;
        before += j < v ? hj : 0;
        nz += hj != 0;
        last = hj != 0 ? hj : last;
      }
      const int stepq = (total - last) / 255;
      if (nz > 1 && stepq > 0) e = min(255, (stepq / 2 + before) / stepq);
    } else if (op == kInvert) {
      e = 255 - v;
    } else if (op == kPosterize) {
      const int bits = min((int)ai, 8);
      e = v & ~((1 << (8 - bits)) - 1);
    } else if (op == kSolarize) {
      e = v < (int)ai ? v : 255 - v;
    } else if (op == kSolarizeAdd) {
      e = v < 128 ? min(255, v + (int)ai) : v;
    } else if (op == kBrightness) {
      e = blend(0.f, (float)v, f);
    } else if (op == kContrast) {
      e = blend((float)level, (float)v, f);
    }
    lut[c * 256 + v] = (uint8_t)e;
  }
}

// in: uint8 [B, H, W, 3]; out: the staging bytes (T = uint8_t, CL, !LAST) or the final tensor.
// hist: this slot's [B, 4, 256].  grid as augment_kernel's: x = chunks of a sample, y = samples.
template <typename T, bool CL, int N, bool LAST>
__global__ __launch_bounds__(kThreads) void rand_apply_kernel(const uint8_t* __restrict__ in, T* __restrict__ out,
                                                              const int* __restrict__ ops,
                                                              const double* __restrict__ args,
                                                              const int* __restrict__ hist,
                                                              const float* __restrict__ table, Fill fill, int B, int n,
                                                              int slot, int H, int W) {
  __shared__ int hs[kHistInts];
  __shared__ uint8_t lut[3 * 256];
  const float* tab = nullptr;
  if constexpr (LAST) {
    __shared__ float tab_s[3 * 256];
    for (int k = threadIdx.x; k < 3 * 256; k += kThreads) tab_s[k] = table[k];
    tab = tab_s;
    __syncthreads();
  }
  const int np = H * W, ne = np * 3;
  const int nv = ne / N;  // N > 1: ne % N == 0
  const int step = gridDim.x * kThreads;
  for (int i = blockIdx.y; i < B; i += gridDim.y) {
    T* o = out + (int64_t)i * ne;
    if (!sample_ok(ops, args, i, n)) {  // block-uniform: nothing read; the last slot marks the sample
      if constexpr (LAST) {
        Run<T, N, true> run;
#pragma unroll
        for (int k = 0; k < N; ++k) run.r[k] = __builtin_nanf("");
        for (int v = blockIdx.x * kThreads + threadIdx.x; v < nv; v += step) run.store(o + (int64_t)v * N);
      }
      continue;
    }
    const int64_t k0 = (int64_t)i * n + slot;
    const int op = ops[k0];
    const double* a = args + k0 * kArgs;
    const uint8_t* s = in + (int64_t)i * ne;
    if (op == kColor) {
      const float f = (float)a[0];
      int r = 0, g = 0, b = 0, gr = 0;
      run_sample<T, CL, N, LAST>(o, tab, H, W, nv, step, [&](int y, int x, int c, bool newpix) {
        if (newpix) {
          const uint8_t* t = s + (y * W + x) * 3;
          r = t[0], g = t[1], b = t[2];
          gr = gray_of(r, g, b);
        }
        return blend((float)gr, (float)pick3(c, r, g, b), f);
      });
    } else if (op == kSharpness) {
      const float f = (float)a[0];
      run_sample<T, CL, N, LAST>(o, tab, H, W, nv, step, [&](int y, int x, int c, bool) {
        // neighbours clamped into the image: every index is in bounds; a border pixel keeps its value
        const int ym = max(y - 1, 0), yp = min(y + 1, H - 1), xm = max(x - 1, 0), xp = min(x + 1, W - 1);
        const bool interior = ym < y && yp > y && xm < x && xp > x;
        auto at = [&](int yy, int xx) -> int { return s[(yy * W + xx) * 3 + c]; };
        const int v = at(y, x);
        const int sum = at(ym, xm) + at(ym, x) + at(ym, xp) + at(y, xm) + 5 * v + at(y, xp) + at(yp, xm) + at(yp, x) +
                        at(yp, xp);
        const int smooth = interior ? (2 * sum + 13) / 26 : v;
        return blend((float)smooth, (float)v, f);
      });
    } else if (op >= kShearX && op <= kRotate) {
      const Mat m{a[0], a[1], a[2], a[3], a[4], a[5]};
      int so = -1;
      run_sample<T, CL, N, LAST>(o, tab, H, W, nv, step, [&](int y, int x, int c, bool newpix) {
        if (newpix) so = affine_source(m, y, x, H, W);
        const int b = s[(so >= 0 ? so : 0) + c];  // in bounds always, replaced after
        return so >= 0 ? b : pick3(c, fill.r, fill.g, fill.b);
      });
    } else {  // a table op, or not applied
      __syncthreads();  // the previous sample's readers of lut
      if (needs_hist(op)) {
        const int* hg = hist + (int64_t)i * kHistInts;
        for (int k = threadIdx.x; k < kHistInts; k += kThreads) hs[k] = hg[k];
        __syncthreads();
      }
      build_tables(lut, hs, op, a[0], np);
      __syncthreads();
      run_sample<T, CL, N, LAST>(o, tab, H, W, nv, step, [&](int y, int x, int c, bool) {
        return (int)lut[c * 256 + s[(y * W + x) * 3 + c]];
      });
    }
  }
}

void check_bytes(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 4 && t.scalar_type() == at::kByte && t.is_contiguous() && t.size(3) == 3,
              what, " must be a dense uint8 [B, H, W, 3] GPU tensor");
  TORCH_CHECK(t.size(1) >= 1 && t.size(1) <= 16384 && t.size(2) >= 1 && t.size(2) <= 16384, what,
              ": image sides must be in [1, 16384]");
  TORCH_CHECK(t.size(1) * t.size(2) * 3 < (int64_t(1) << 31) && t.size(0) < (int64_t(1) << 31), what,
              ": sample or batch too large");
}

// blocks of a pass over `nv` work items per sample: at most ~2048, 32 chunks per sample, the rest over the batch
dim3 pass_grid(int64_t nv, int64_t B, int64_t max_chunks = 32) {
  const int64_t gx = std::min<int64_t>((nv + kThreads - 1) / kThreads, max_chunks);
  return dim3((unsigned)gx, (unsigned)std::min<int64_t>(B, std::max<int64_t>(1, 2048 / gx)));
}

}  // namespace

// src: dense uint8 [B, Hs, Ws, 3] on the GPU; plan: int32 [B, 5] rows (x0, y0, cw, ch, flip) on
// src's device (augment_batch's); a new uint8 [B, out_h, out_w, 3].
at::Tensor crop_bytes(const at::Tensor& src, const at::Tensor& plan, int64_t out_h, int64_t out_w) {
  check_bytes(src, "crop_bytes: src");
  const int64_t B = src.size(0), Hs = src.size(1), Ws = src.size(2);
  TORCH_CHECK(plan.is_cuda() && plan.device() == src.device() && plan.scalar_type() == at::kInt && plan.dim() == 2 &&
                  plan.size(0) == B && plan.size(1) == 5 && plan.is_contiguous(),
              "crop_bytes: plan must be a contiguous int32 [B, 5] tensor on src's device");
  TORCH_CHECK(out_h >= 1 && out_h <= 16384 && out_w >= 1 && out_w <= 16384 && out_h * out_w * 3 < (int64_t(1) << 31),
              "crop_bytes: output sides must be in [1, 16384]");
  auto out = at::empty({B, out_h, out_w, 3}, src.options());
  if (B == 0) return out;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(crop_bytes_kernel, pass_grid(out_h * out_w, B), dim3(kThreads), 0, stream,
                     src.data_ptr<uint8_t>(), plan.data_ptr<int>(), out.data_ptr<uint8_t>(), (int)B, (int)Hs, (int)Ws,
                     (int)out_h, (int)out_w);
  DMP_HIP_CHECK(hipGetLastError());
  return out;
}

// u8: dense uint8 [B, H, W, 3] on the GPU (never written); ops: int32 [B, n], args: float64
// [B, n, 6], table: fp32 [3, 256], all on u8's device; hist_slots: n flags, non-zero where the
// slot's ops include one that needs the histograms; fill: the affine ops' colour, three bytes.
// A new [B, 3, H, W] bf16 / fp32, dense channels-last or NCHW.
at::Tensor rand_augment_apply(const at::Tensor& u8, const at::Tensor& ops, const at::Tensor& args,
                              const std::vector<int64_t>& hist_slots, const std::vector<int64_t>& fill,
                              const at::Tensor& table, at::ScalarType dtype, bool channels_last) {
  check_bytes(u8, "rand_augment_apply: u8");
  const int64_t B = u8.size(0), H = u8.size(1), W = u8.size(2);
  TORCH_CHECK(ops.dim() == 2 && ops.size(0) == B, "rand_augment_apply: ops must be int32 [B, n]");
  const int64_t n = ops.size(1);
  TORCH_CHECK(n >= 1 && n <= kMaxSlots, "rand_augment_apply: 1 to ", kMaxSlots, " op slots, got ", n);
  TORCH_CHECK(ops.is_cuda() && ops.device() == u8.device() && ops.scalar_type() == at::kInt && ops.is_contiguous(),
              "rand_augment_apply: ops must be a contiguous int32 [B, n] tensor on u8's device");
  TORCH_CHECK(args.is_cuda() && args.device() == u8.device() && args.scalar_type() == at::kDouble &&
                  args.is_contiguous() && args.dim() == 3 && args.size(0) == B && args.size(1) == n &&
                  args.size(2) == kArgs,
              "rand_augment_apply: args must be a contiguous float64 [B, n, 6] tensor on u8's device");
  TORCH_CHECK(table.is_cuda() && table.device() == u8.device() && table.scalar_type() == at::kFloat &&
                  table.is_contiguous() && table.dim() == 2 && table.size(0) == 3 && table.size(1) == 256,
              "rand_augment_apply: table must be a contiguous fp32 [3, 256] tensor on u8's device");
  TORCH_CHECK((int64_t)hist_slots.size() == n, "rand_augment_apply: hist_slots needs one flag per slot");
  TORCH_CHECK(fill.size() == 3, "rand_augment_apply: fill needs three entries");
  for (int64_t v : fill) TORCH_CHECK(v >= 0 && v <= 255, "rand_augment_apply: fill entries must be bytes");
  TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16, "rand_augment_apply: dtype must be fp32 or bf16");
  auto out = at::empty({B, 3, H, W}, u8.options().dtype(dtype),
                       channels_last ? at::MemoryFormat::ChannelsLast : at::MemoryFormat::Contiguous);
  if (B == 0) return out;
  const int64_t np = H * W, ne = np * 3;
  auto stream = at::hip::getCurrentHIPStream();
  const Fill fl{(int)fill[0], (int)fill[1], (int)fill[2]};
  bool any_hist = false;
  for (int64_t v : hist_slots) any_hist = any_hist || v != 0;
  at::Tensor hist;
  if (any_hist) {
    hist = at::empty({n, B, 4, 256}, u8.options().dtype(at::kInt));
    DMP_HIP_CHECK(hipMemsetAsync(hist.data_ptr(), 0, (size_t)hist.numel() * sizeof(int), stream));
  }
  at::Tensor stage[2];  // ping-pong: slot k reads what slot k - 1 wrote, never its own output
  const uint8_t* cur = u8.data_ptr<uint8_t>();
  const int* opp = ops.data_ptr<int>();
  const double* argp = args.data_ptr<double>();
  const float* tabp = table.data_ptr<float>();
  for (int64_t slot = 0; slot < n; ++slot) {
    const int* hp = nullptr;
    if (hist_slots[slot] != 0) {
      int* h = hist.data_ptr<int>() + slot * B * kHistInts;
      // every block adds up to 1024 bins to global memory: as few chunks per sample as still fill the GPU
      const int64_t chunks = std::min<int64_t>(32, std::max<int64_t>(4, 2048 / B));
      hipLaunchKernelGGL(rand_hist_kernel, pass_grid(np, B, chunks), dim3(kThreads), 0, stream, cur, opp, argp, h,
                         (int)B, (int)n, (int)slot, (int)np);
      hp = h;
    } else if (any_hist) {
      hp = hist.data_ptr<int>() + slot * B * kHistInts;  // zeros: an unannounced histogram op is the identity
    }
    auto launch = [&](auto ttag, auto ltag, auto ntag, auto lasttag, void* dst) {
      using T = decltype(ttag);
      constexpr int N = decltype(ntag)::value;
      hipLaunchKernelGGL((rand_apply_kernel<T, decltype(ltag)::value, N, decltype(lasttag)::value>),
                         pass_grid(ne / N, B), dim3(kThreads), 0, stream, cur, reinterpret_cast<T*>(dst), opp, argp,
                         hp, tabp, fl, (int)B, (int)n, (int)slot, (int)H, (int)W);
    };
    if (slot + 1 < n) {
      at::Tensor& st = stage[slot & 1];
      if (!st.defined()) st = at::empty_like(u8);
      if (ne % 16 == 0) launch(uint8_t{}, std::true_type{}, std::integral_constant<int, 16>{}, std::false_type{}, st.data_ptr());
      else launch(uint8_t{}, std::true_type{}, std::integral_constant<int, 1>{}, std::false_type{}, st.data_ptr());
      cur = st.data_ptr<uint8_t>();
    } else {
      auto by_layout = [&](auto ttag, auto ntag) {
        const bool vec = ne % decltype(ntag)::value == 0 && reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0;
        if (channels_last && vec) launch(ttag, std::true_type{}, ntag, std::true_type{}, out.data_ptr());
        else if (channels_last) launch(ttag, std::true_type{}, std::integral_constant<int, 1>{}, std::true_type{}, out.data_ptr());
        else if (vec) launch(ttag, std::false_type{}, ntag, std::true_type{}, out.data_ptr());
        else launch(ttag, std::false_type{}, std::integral_constant<int, 1>{}, std::true_type{}, out.data_ptr());
      };
      if (dtype == at::kFloat) by_layout(float{}, std::integral_constant<int, 4>{});
      else by_layout(__bf16{}, std::integral_constant<int, 8>{});
    }
    DMP_HIP_CHECK(hipGetLastError());
  }
  return out;
}

}  // namespace dmp
