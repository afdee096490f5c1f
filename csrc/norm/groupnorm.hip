// GroupNorm (+ residual) (+ ReLU / ReLU6) on channels-last rows x [N, HW, C]
// for gfx950, forward and backward, bf16 or fp32 activations, fp32 parameters.
//
// Capability: torch.nn.GroupNorm followed by an add and a (clipped) ReLU, as
// the GN variants of MobileNetV2 and ResNet use it (ops/groupnorm.py).
//
// Design.  In channels-last memory the G groups of a sample are independent
// column bands: a block owns (sample n, W = k * cg adjacent channels, a run of
// rows) and never talks to another block.
//   * Threads form a (row lane, 8-channel vector) grid: with SV = W / 8
//     vectors per row segment, thread t serves vector t % SV of the rows
//     t / SV, t / SV + RS, ... (RS = 256 / SV).  A thread keeps its 8 channels
//     for the whole kernel, so gamma / beta / mean / rstd live in registers.
//   * Resident path (one run of rows = the whole sample): the slab
//     HW x W goes into LDS once with 16-byte loads, each thread re-reading only
//     what it wrote (no barrier on the slab).  The mean comes from a first LDS
//     pass, the variance from a second one as the mean of squared deviations,
//     the apply from a third: HBM sees one read of x and one write of y.
//     Backward keeps the x slab and the masked gradient dz: one read of x, dy
//     (and y when the mask comes from it), one write of dx.
//   * Streamed path (the slab does not fit at one group-vector per block):
//     rows are split into chunks of rows_per_block; the SAME kernels run in
//     "stats" mode on a chunk (two LDS passes -> per-chunk mean and M2, or the
//     two backward sums), a one-thread-per-(n, g) kernel folds the chunks in
//     index order (Chan's update forward), and the kernels run again in
//     "apply" mode re-reading x.
//   * Group sums: per-thread partials -> LDS [row lane][slot]; wave w folds
//     groups w, w + 4, ...: lane l adds entries l, l + 64, ... in order, then
//     an xor butterfly.  Fixed order everywhere, no atomics: two runs are
//     bit-identical.
//   * cg in {1, 2, 4}: one vector spans 8 / cg groups; the thread keeps that
//     many sub-sums (template CGS = channels per sub-sum).
//   * dgamma / dbeta: per-thread column sums folded over the row lanes through
//     LDS into one [2C] partial row per (sample, chunk), then colreduce.
//
// LDS budget: kGnSlab = 64 KB of slab per forward block (+ 12 KB of reduce and
// statistics words = 76 KB, two blocks per CU); backward holds two slabs
// (140 KB, one block per CU).  Slabs of at most kGnSlabSmall = 16 KB run on
// instantiations that declare only that much, for occupancy.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "../colreduce.h"
#include "../api.h"
#include "../common.h"

namespace dmp {
namespace {

constexpr int kGnThreads = 256;
constexpr int kGnSlab = 64 * 1024;       // resident slab budget per block (bytes)
constexpr int kGnSlabSmall = 16 * 1024;  // small-slab instantiations; streamed chunk size
constexpr int kGnMaxGroups = 512;        // groups per block (statistics words in LDS)
constexpr int kGnRed = 2048;             // reduce words: 256 threads x 8
constexpr int kGnSegBytes = 128;         // preferred row-segment width
constexpr int kGnMaxCg = 2048;           // SV = W / 8 <= 256

enum { kResident = 0, kStats = 1, kApply = 2 };

struct GnGeom {
  int HW, C, G, cg;
  int W;       // channels per block
  int segs;    // ceil(C / W)
  int rpb;     // rows per block
  int chunks;  // ceil(HW / rpb); 1 = resident
};

GnGeom gn_geom(int64_t HW, int64_t C, int64_t G, int sz) {
  GnGeom g;
  g.HW = (int)HW; g.C = (int)C; g.G = (int)G; g.cg = (int)(C / G);
  const int64_t unit = g.cg >= 8 ? g.cg : 8;  // whole groups and whole vectors
  int64_t W = std::min<int64_t>(C, (kGnSegBytes / sz + unit - 1) / unit * unit);
  while (HW * W * sz > kGnSlab && W > unit) W -= unit;
  if (HW * W * sz <= kGnSlab) {
    g.rpb = (int)std::max<int64_t>(HW, 1);
    g.chunks = 1;
  } else {
    W = g.cg >= 8 ? std::max<int64_t>(g.cg, kGnMaxGroups / g.cg * g.cg) : kGnMaxGroups;
    W = std::min<int64_t>(W, C);
    g.rpb = (int)std::max<int64_t>(1, kGnSlabSmall / (W * sz));
    g.chunks = (int)((HW + g.rpb - 1) / g.rpb);
  }
  g.W = (int)W;
  g.segs = (int)((C + W - 1) / W);
  return g;
}

// A thread's place in its block's (row lane, vector) grid.
struct GnPos {
  int n, chunk, r0, r1, c0, nvec, SV, RS, col, rl;
  bool active;
};

__device__ __forceinline__ GnPos gn_pos(const GnGeom& g) {
  GnPos p;
  const int bps = g.segs * g.chunks;
  p.n = blockIdx.x / bps;
  const int rem = blockIdx.x - p.n * bps;
  p.chunk = rem / g.segs;
  const int seg = rem - p.chunk * g.segs;
  p.r0 = p.chunk * g.rpb;
  p.r1 = min(g.HW, p.r0 + g.rpb);
  p.c0 = seg * g.W;
  p.SV = g.W / 8;
  p.nvec = min(p.SV, (g.C - p.c0) / 8);
  p.RS = kGnThreads / p.SV;
  p.col = threadIdx.x % p.SV;
  p.rl = threadIdx.x / p.SV;
  p.active = p.rl < p.RS && p.col < p.nvec;
  return p;
}

// out[q] = scale * (sum of v over group q of the block), q < kb.  Slots of a
// thread: col * NSUB + j; group q owns slots q * spg ... q * spg + spg - 1.
template <int NSUB>
__device__ __forceinline__ void gn_fold(float* red, float* out, const float (&v)[NSUB], const GnPos& p,
                                        int spg, int kb, float scale) {
  const int stride = p.SV * NSUB;
  if (p.active) {
#pragma unroll
    for (int j = 0; j < NSUB; ++j) red[p.rl * stride + p.col * NSUB + j] = v[j];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, E = p.RS * spg;
  for (int q = threadIdx.x >> 6; q < kb; q += kGnThreads / 64) {
    float a = 0.f;
    for (int e = lane; e < E; e += 64) {
      const int rl = e / spg;
      a += red[rl * stride + q * spg + (e - rl * spg)];
    }
    a = wave_sum(a);
    if (lane == 0) out[q] = a * scale;
  }
  __syncthreads();
}

// part[c0 + e] = sum over the row lanes of acc (a thread's 8 column sums), e < nvec * 8.
__device__ __forceinline__ void gn_fold_cols(float* red, float* part, const float (&acc)[8], const GnPos& p) {
  if (p.active) {
#pragma unroll
    for (int i = 0; i < 8; ++i) red[(p.rl * p.SV + p.col) * 8 + i] = acc[i];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < p.nvec * 8; e += kGnThreads) {
    float a = 0.f;
    for (int rl = 0; rl < p.RS; ++rl) a += red[rl * p.SV * 8 + e];
    part[p.c0 + e] = a;
  }
  __syncthreads();
}

// The LDS slab: 8-element vectors of T at index i; fp32 as two 16-byte planes.
template <typename T>
__device__ __forceinline__ void slab_put(char* slab, int i, int plane, const float (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    Vec16<__bf16>::store(reinterpret_cast<__bf16*>(slab) + (int64_t)i * 8, v);
  } else {
    float a[4] = {v[0], v[1], v[2], v[3]}, b[4] = {v[4], v[5], v[6], v[7]};
    Vec16<float>::store(reinterpret_cast<float*>(slab) + (int64_t)i * 4, a);
    Vec16<float>::store(reinterpret_cast<float*>(slab) + (int64_t)(plane + i) * 4, b);
  }
}
template <typename T>
__device__ __forceinline__ void slab_get(const char* slab, int i, int plane, float (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    Vec16<__bf16>::load(reinterpret_cast<const __bf16*>(slab) + (int64_t)i * 8, v);
  } else {
    float a[4], b[4];
    Vec16<float>::load(reinterpret_cast<const float*>(slab) + (int64_t)i * 4, a);
    Vec16<float>::load(reinterpret_cast<const float*>(slab) + (int64_t)(plane + i) * 4, b);
#pragma unroll
    for (int i2 = 0; i2 < 4; ++i2) { v[i2] = a[i2]; v[4 + i2] = b[i2]; }
  }
}

// The forward's pre-activation value; backward re-derives the mask with the same expression.
__device__ __forceinline__ float gn_affine(float x, float m, float a, float b) { return fmaf(x - m, a, b); }

// y = act((x - mean) * rstd * gamma + beta [+ res]).
//   kResident: statistics and apply from the LDS slab; writes mean / rstd.
//   kStats:    per-chunk (mean, M2) of every group -> ws[n][chunk][G][2].
//   kApply:    mean / rstd read back, x re-read from memory.
template <typename T, int CGS, int MODE, int SLAB>
__global__ __launch_bounds__(kGnThreads) void gn_fwd_kernel(
    const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
    const T* __restrict__ res, GnGeom g, float eps, int act, float clip, T* __restrict__ y,
    float* __restrict__ mean_io, float* __restrict__ rstd_io, float* __restrict__ ws) {
  constexpr int NSUB = 8 / CGS;
  __shared__ __attribute__((aligned(16))) char slab[SLAB > 0 ? SLAB : 16];
  __shared__ float red[kGnRed];
  __shared__ float mean_s[kGnMaxGroups], rstd_s[kGnMaxGroups];
  const GnPos p = gn_pos(g);
  const int spg = max(1, g.cg / 8);
  const int kb = p.nvec * NSUB / spg, g0 = p.c0 / g.cg;
  const int rows = p.r1 - p.r0, plane = rows * p.SV;
  const float cnt = (float)rows * (float)g.cg;
  const int64_t base = ((int64_t)p.n * g.HW) * g.C + p.c0 + p.col * 8;
  const int q0 = p.col * NSUB / spg;  // group of sub-sum j: q0 + j (NSUB > 1 has spg = 1)

  if constexpr (MODE != kApply) {
    float s[NSUB];
#pragma unroll
    for (int j = 0; j < NSUB; ++j) s[j] = 0.f;
    if (p.active) {
#pragma unroll 4
      for (int r = p.r0 + p.rl; r < p.r1; r += p.RS) {
        float v[8];
        load8<T>(x + base + (int64_t)r * g.C, v);
        slab_put<T>(slab, (r - p.r0) * p.SV + p.col, plane, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i / CGS] += v[i];
      }
    }
    gn_fold<NSUB>(red, mean_s, s, p, spg, kb, 1.f / cnt);
    float m[NSUB], d2[NSUB];
#pragma unroll
    for (int j = 0; j < NSUB; ++j) { m[j] = p.active ? mean_s[q0 + j] : 0.f; d2[j] = 0.f; }
    if (p.active) {
      for (int r = p.r0 + p.rl; r < p.r1; r += p.RS) {
        float v[8];
        slab_get<T>(slab, (r - p.r0) * p.SV + p.col, plane, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float d = v[i] - m[i / CGS];
          d2[i / CGS] = fmaf(d, d, d2[i / CGS]);
        }
      }
    }
    gn_fold<NSUB>(red, rstd_s, d2, p, spg, kb, 1.f);  // M2 for now
    if constexpr (MODE == kStats) {
      for (int q = threadIdx.x; q < kb; q += kGnThreads) {
        float* o = ws + (((int64_t)p.n * g.chunks + p.chunk) * g.G + g0 + q) * 2;
        o[0] = mean_s[q];
        o[1] = rstd_s[q];
      }
      return;
    }
    for (int q = threadIdx.x; q < kb; q += kGnThreads) {
      const float rs = rsqrtf(rstd_s[q] / cnt + eps);
      rstd_s[q] = rs;
      mean_io[(int64_t)p.n * g.G + g0 + q] = mean_s[q];
      rstd_io[(int64_t)p.n * g.G + g0 + q] = rs;
    }
    __syncthreads();
  } else {
    for (int q = threadIdx.x; q < kb; q += kGnThreads) {
      mean_s[q] = mean_io[(int64_t)p.n * g.G + g0 + q];
      rstd_s[q] = rstd_io[(int64_t)p.n * g.G + g0 + q];
    }
    __syncthreads();
  }
  if (!p.active) return;
  float ga[8], gb[8], m[NSUB];
  load8<float>(w + p.c0 + p.col * 8, ga);
  load8<float>(b + p.c0 + p.col * 8, gb);
#pragma unroll
  for (int j = 0; j < NSUB; ++j) m[j] = mean_s[q0 + j];
#pragma unroll
  for (int i = 0; i < 8; ++i) ga[i] *= rstd_s[q0 + i / CGS];
#pragma unroll 2
  for (int r = p.r0 + p.rl; r < p.r1; r += p.RS) {
    float v[8], o[8];
    if constexpr (MODE == kApply) load8<T>(x + base + (int64_t)r * g.C, v);
    else slab_get<T>(slab, (r - p.r0) * p.SV + p.col, plane, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = gn_affine(v[i], m[i / CGS], ga[i], gb[i]);
    if (res != nullptr) {
      float rv[8];
      load8<T>(res + base + (int64_t)r * g.C, rv);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] += rv[i];
    }
    if (act) {
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = fminf(fmaxf(o[i], 0.f), clip);
    }
    store8<T>(y + base + (int64_t)r * g.C, o);
  }
}

// Streamed forward: fold the chunks' (count, mean, M2) of group (n, g) in chunk order.
__global__ void gn_fwd_finalize_kernel(const float* __restrict__ ws, int64_t ng, GnGeom g, float eps,
                                       float* __restrict__ mean, float* __restrict__ rstd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ng) return;
  const int64_t n = i / g.G;
  const int gi = (int)(i - n * g.G);
  float na = 0.f, ma = 0.f, m2 = 0.f;
  for (int c = 0; c < g.chunks; ++c) {
    const float* o = ws + ((n * g.chunks + c) * g.G + gi) * 2;
    const float nb = (float)(min(g.HW, (c + 1) * g.rpb) - c * g.rpb) * (float)g.cg;
    const float d = o[0] - ma, nt = na + nb;
    ma += d * (nb / nt);
    m2 += o[1] + d * d * (na * nb / nt);
    na = nt;
  }
  mean[i] = ma;
  rstd[i] = rsqrtf(m2 / na + eps);
}

// dz = dy masked by the activation; dx = rstd * (dz gamma - c1 - xhat c2) with
// c1 = mean(dz gamma), c2 = mean(dz gamma xhat) over the group.
//   kResident: x and dz slabs in LDS between the sums and the apply.
//   kStats:    the chunk's two sums -> ws[n][chunk][G][2] (no slab).
//   kApply:    c1 / c2 read from csum[n][G][2]; x, dy (and y) re-read.
// kResident and kStats also write dres = dz and the chunk's dgamma / dbeta row.
template <typename T, int CGS, int MODE, int SLAB>
__global__ __launch_bounds__(kGnThreads) void gn_bwd_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ y,
    const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ mean,
    const float* __restrict__ rstd, GnGeom g, int act, float clip, T* __restrict__ dx,
    T* __restrict__ dres, float* __restrict__ part, float* __restrict__ ws,
    const float* __restrict__ csum) {
  constexpr int NSUB = 8 / CGS;
  __shared__ __attribute__((aligned(16))) char slab[SLAB > 0 ? 2 * SLAB : 16];
  __shared__ float red[kGnRed];
  __shared__ float mean_s[kGnMaxGroups], rstd_s[kGnMaxGroups], c1_s[kGnMaxGroups], c2_s[kGnMaxGroups];
  const GnPos p = gn_pos(g);
  const int spg = max(1, g.cg / 8);
  const int kb = p.nvec * NSUB / spg, g0 = p.c0 / g.cg;
  const int rows = p.r1 - p.r0, plane = rows * p.SV;
  const int64_t base = ((int64_t)p.n * g.HW) * g.C + p.c0 + p.col * 8;
  const int q0 = p.col * NSUB / spg;
  char* slab_dz = slab + (SLAB > 0 ? SLAB : 0);

  for (int q = threadIdx.x; q < kb; q += kGnThreads) {
    mean_s[q] = mean[(int64_t)p.n * g.G + g0 + q];
    rstd_s[q] = rstd[(int64_t)p.n * g.G + g0 + q];
    if constexpr (MODE == kApply) {
      c1_s[q] = csum[((int64_t)p.n * g.G + g0 + q) * 2];
      c2_s[q] = csum[((int64_t)p.n * g.G + g0 + q) * 2 + 1];
    }
  }
  __syncthreads();
  float gw[8], gb[8], ga[8], m[NSUB], rs[NSUB];
#pragma unroll
  for (int i = 0; i < 8; ++i) { gw[i] = 0.f; gb[i] = 0.f; }
#pragma unroll
  for (int j = 0; j < NSUB; ++j) { m[j] = 0.f; rs[j] = 0.f; }
  if (p.active) {
    load8<float>(w + p.c0 + p.col * 8, gw);
    load8<float>(b + p.c0 + p.col * 8, gb);
#pragma unroll
    for (int j = 0; j < NSUB; ++j) { m[j] = mean_s[q0 + j]; rs[j] = rstd_s[q0 + j]; }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) ga[i] = gw[i] * rs[i / CGS];
  // dz of one row vector: the mask from y when it was saved, else from x as the forward formed it
  auto masked = [&](int r, const float (&xv)[8], float (&dz)[8]) {
    load8<T>(dy + base + (int64_t)r * g.C, dz);
    if (act) {
      float t[8];
      if (y != nullptr) {
        load8<T>(y + base + (int64_t)r * g.C, t);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = gn_affine(xv[i], m[i / CGS], ga[i], gb[i]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) dz[i] = (t[i] > 0.f && t[i] < clip) ? dz[i] : 0.f;
    }
  };

  if constexpr (MODE != kApply) {
    float s1[NSUB], s2[NSUB], accw[8], accb[8];
#pragma unroll
    for (int j = 0; j < NSUB; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
#pragma unroll
    for (int i = 0; i < 8; ++i) { accw[i] = 0.f; accb[i] = 0.f; }
    if (p.active) {
#pragma unroll 2
      for (int r = p.r0 + p.rl; r < p.r1; r += p.RS) {
        float xv[8], dz[8];
        load8<T>(x + base + (int64_t)r * g.C, xv);
        masked(r, xv, dz);
        if (dres != nullptr) store8<T>(dres + base + (int64_t)r * g.C, dz);
        if constexpr (MODE == kResident) {
          slab_put<T>(slab, (r - p.r0) * p.SV + p.col, plane, xv);
          slab_put<T>(slab_dz, (r - p.r0) * p.SV + p.col, plane, dz);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float xh = (xv[i] - m[i / CGS]) * rs[i / CGS], dg = dz[i] * gw[i];
          s1[i / CGS] += dg;
          s2[i / CGS] = fmaf(dg, xh, s2[i / CGS]);
          accw[i] = fmaf(dz[i], xh, accw[i]);
          accb[i] += dz[i];
        }
      }
    }
    const float inv = MODE == kResident ? 1.f / ((float)g.HW * (float)g.cg) : 1.f;
    gn_fold<NSUB>(red, c1_s, s1, p, spg, kb, inv);
    gn_fold<NSUB>(red, c2_s, s2, p, spg, kb, inv);
    float* prow = part + ((int64_t)p.n * g.chunks + p.chunk) * 2 * g.C;
    gn_fold_cols(red, prow, accw, p);
    gn_fold_cols(red, prow + g.C, accb, p);
    if constexpr (MODE == kStats) {
      for (int q = threadIdx.x; q < kb; q += kGnThreads) {
        float* o = ws + (((int64_t)p.n * g.chunks + p.chunk) * g.G + g0 + q) * 2;
        o[0] = c1_s[q];
        o[1] = c2_s[q];
      }
      return;
    }
  }
  if (!p.active) return;
  float c1[NSUB], c2[NSUB];
#pragma unroll
  for (int j = 0; j < NSUB; ++j) { c1[j] = c1_s[q0 + j]; c2[j] = c2_s[q0 + j]; }
#pragma unroll 2
  for (int r = p.r0 + p.rl; r < p.r1; r += p.RS) {
    float xv[8], dz[8], o[8];
    if constexpr (MODE == kApply) {
      load8<T>(x + base + (int64_t)r * g.C, xv);
      masked(r, xv, dz);
    } else {
      slab_get<T>(slab, (r - p.r0) * p.SV + p.col, plane, xv);
      slab_get<T>(slab_dz, (r - p.r0) * p.SV + p.col, plane, dz);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float xh = (xv[i] - m[i / CGS]) * rs[i / CGS];
      o[i] = rs[i / CGS] * (dz[i] * gw[i] - c1[i / CGS] - xh * c2[i / CGS]);
    }
    store8<T>(dx + base + (int64_t)r * g.C, o);
  }
}

// Streamed backward: csum[n][g] = (sum over chunks, in order) / (HW cg), both sums.
__global__ void gn_bwd_finalize_kernel(const float* __restrict__ ws, int64_t ng, GnGeom g,
                                       float* __restrict__ csum) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ng) return;
  const int64_t n = i / g.G;
  const int gi = (int)(i - n * g.G);
  float a = 0.f, c = 0.f;
  for (int k = 0; k < g.chunks; ++k) {
    const float* o = ws + ((n * g.chunks + k) * g.G + gi) * 2;
    a += o[0];
    c += o[1];
  }
  const float inv = 1.f / ((float)g.HW * (float)g.cg);
  csum[i * 2] = a * inv;
  csum[i * 2 + 1] = c * inv;
}

template <typename T>
using FwdFn = void (*)(const T*, const float*, const float*, const T*, GnGeom, float, int, float, T*,
                       float*, float*, float*);
template <typename T>
using BwdFn = void (*)(const T*, const T*, const T*, const float*, const float*, const float*,
                       const float*, GnGeom, int, float, T*, T*, float*, float*, const float*);

template <typename T, int MODE, int SLAB>
FwdFn<T> fwd_for(int cg) {
  return cg >= 8 ? gn_fwd_kernel<T, 8, MODE, SLAB> : cg == 4 ? gn_fwd_kernel<T, 4, MODE, SLAB>
       : cg == 2 ? gn_fwd_kernel<T, 2, MODE, SLAB> : gn_fwd_kernel<T, 1, MODE, SLAB>;
}
template <typename T, int MODE, int SLAB>
BwdFn<T> bwd_for(int cg) {
  return cg >= 8 ? gn_bwd_kernel<T, 8, MODE, SLAB> : cg == 4 ? gn_bwd_kernel<T, 4, MODE, SLAB>
       : cg == 2 ? gn_bwd_kernel<T, 2, MODE, SLAB> : gn_bwd_kernel<T, 1, MODE, SLAB>;
}
// the resident instantiation whose slab array is just large enough
bool small_slab(const GnGeom& g, int sz) { return (int64_t)g.HW * g.W * sz <= kGnSlabSmall; }

void check_gn(const at::Tensor& t, const at::Tensor& x, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == x.scalar_type() &&
                  t.sizes() == x.sizes() && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "groupnorm: ", name, " must be a contiguous 16-byte aligned GPU tensor of x's shape and dtype");
}

GnGeom checked_geom(const at::Tensor& x, int64_t G) {
  TORCH_CHECK(x.dim() == 3, "groupnorm: x must be [N, HW, C]");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat, "groupnorm: bf16 or fp32");
  check_gn(x, x, "x");
  TORCH_CHECK(groupnorm_supported(x.size(2), G), "groupnorm: unsupported (C, G) = (", x.size(2), ", ", G, ")");
  TORCH_CHECK(x.size(1) < (1 << 24), "groupnorm: too many rows per sample");
  const GnGeom g = gn_geom(x.size(1), x.size(2), G, (int)x.element_size());
  TORCH_CHECK(x.size(0) * (int64_t)g.segs * g.chunks < (int64_t(1) << 31), "groupnorm: too many blocks");
  return g;
}

// fp32 [C] parameter, or ones / zeros for an absent one (branch-free kernel loads)
at::Tensor param_or(const c10::optional<at::Tensor>& p, const at::Tensor& x, int64_t C, bool one) {
  if (p.has_value() && p->defined()) {
    TORCH_CHECK(p->is_cuda() && p->is_contiguous() && p->numel() == C && p->scalar_type() == at::kFloat,
                "groupnorm: weight / bias must be contiguous fp32 [C]");
    return *p;
  }
  const auto o = x.options().dtype(at::kFloat);
  return one ? at::ones({C}, o) : at::zeros({C}, o);
}

}  // namespace

bool groupnorm_supported(int64_t C, int64_t G) {
  if (C <= 0 || G <= 0 || C % 8 != 0 || C % G != 0) return false;
  const int64_t cg = C / G;
  return cg <= kGnMaxCg && (cg % 8 == 0 || cg == 1 || cg == 2 || cg == 4);
}

std::map<std::string, int64_t> groupnorm_plan(int64_t N, int64_t HW, int64_t C, int64_t G,
                                              at::ScalarType dtype) {
  TORCH_CHECK(groupnorm_supported(C, G), "groupnorm_plan: unsupported (C, G)");
  const int sz = dtype == at::kBFloat16 ? 2 : 4;
  const GnGeom g = gn_geom(HW, C, G, sz);
  const int64_t stat = 4 * (kGnRed + 2 * kGnMaxGroups), slab = (int64_t)std::min(g.rpb, g.HW) * g.W * sz;
  const int64_t decl = g.chunks > 1 || slab <= kGnSlabSmall ? kGnSlabSmall : kGnSlab;
  return {{"path", g.chunks > 1 ? 1 : 0},
          {"groups_per_block", g.W / g.cg},
          {"blocks", N * g.segs * g.chunks},
          {"rows_per_block", g.rpb},
          {"segment_channels", g.W},
          {"slab_bytes", slab},
          {"lds_bytes", decl + stat},
          {"lds_bytes_backward", (g.chunks > 1 ? 16 : 2 * decl) + stat + 8 * kGnMaxGroups}};
}

// Returns (y, mean [N, G], rstd [N, G]).
std::vector<at::Tensor> groupnorm_forward(const at::Tensor& x, const c10::optional<at::Tensor>& weight,
                                          const c10::optional<at::Tensor>& bias,
                                          const c10::optional<at::Tensor>& residual, int64_t G,
                                          double eps, bool act, double clip) {
  const GnGeom g = checked_geom(x, G);
  const int64_t N = x.size(0), C = x.size(2);
  const bool hr = residual.has_value() && residual->defined();
  if (hr) check_gn(*residual, x, "residual");
  auto y = at::empty_like(x);
  auto mean = at::empty({N, G}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({N, G}, x.options().dtype(at::kFloat));
  if (x.numel() == 0) return {y, mean, rstd};
  const at::Tensor wt = param_or(weight, x, C, true), bt = param_or(bias, x, C, false);
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid((unsigned)(N * g.segs * g.chunks)), block(kGnThreads);
  const bool streamed = g.chunks > 1;
  at::Tensor ws;
  if (streamed) ws = at::empty({N, g.chunks, G, 2}, mean.options());
  auto run = [&](auto tag) {
    using T = decltype(tag);
    const T* xp = reinterpret_cast<const T*>(x.data_ptr());
    const T* rp = hr ? reinterpret_cast<const T*>(residual->data_ptr()) : nullptr;
    T* yp = reinterpret_cast<T*>(y.data_ptr());
    const float *wp = wt.data_ptr<float>(), *bp = bt.data_ptr<float>();
    float *mp = mean.data_ptr<float>(), *sp = rstd.data_ptr<float>();
    if (!streamed) {
      const FwdFn<T> k = small_slab(g, sizeof(T)) ? fwd_for<T, kResident, kGnSlabSmall>(g.cg)
                                                  : fwd_for<T, kResident, kGnSlab>(g.cg);
      hipLaunchKernelGGL(k, grid, block, 0, stream, xp, wp, bp, rp, g, (float)eps, (int)act, (float)clip, yp,
                         mp, sp, (float*)nullptr);
      return;
    }
    hipLaunchKernelGGL((fwd_for<T, kStats, kGnSlabSmall>(g.cg)), grid, block, 0, stream, xp, wp, bp, rp, g,
                       (float)eps, (int)act, (float)clip, yp, mp, sp, ws.data_ptr<float>());
    hipLaunchKernelGGL(gn_fwd_finalize_kernel, dim3((unsigned)((N * G + 255) / 256)), dim3(256), 0, stream,
                       ws.data_ptr<float>(), N * G, g, (float)eps, mp, sp);
    hipLaunchKernelGGL((fwd_for<T, kApply, 0>(g.cg)), grid, block, 0, stream, xp, wp, bp, rp, g, (float)eps,
                       (int)act, (float)clip, yp, mp, sp, (float*)nullptr);
  };
  if (x.scalar_type() == at::kBFloat16) run(__bf16{}); else run(float{});
  return {y, mean, rstd};
}

// Returns (dx, dgamma, dbeta [, dres = dz when want_dres]); dgamma / dbeta in param_dtype.
// y: the saved forward output when the mask comes from it (a residual was added), else none.
std::vector<at::Tensor> groupnorm_backward(const at::Tensor& dy, const at::Tensor& x,
                                           const c10::optional<at::Tensor>& y,
                                           const c10::optional<at::Tensor>& weight,
                                           const c10::optional<at::Tensor>& bias, const at::Tensor& mean,
                                           const at::Tensor& rstd, int64_t G, bool act, double clip,
                                           bool want_dres, at::ScalarType param_dtype) {
  const GnGeom g = checked_geom(x, G);
  const int64_t N = x.size(0), C = x.size(2);
  check_gn(dy, x, "dy");
  const bool hy = y.has_value() && y->defined();
  if (hy) check_gn(*y, x, "y");
  TORCH_CHECK(mean.is_cuda() && mean.is_contiguous() && mean.scalar_type() == at::kFloat && mean.numel() == N * G &&
                  rstd.is_cuda() && rstd.is_contiguous() && rstd.scalar_type() == at::kFloat && rstd.numel() == N * G,
              "groupnorm: mean / rstd must be contiguous fp32 [N, G]");
  TORCH_CHECK(param_dtype == at::kFloat || param_dtype == at::kBFloat16, "groupnorm: param_dtype fp32 or bf16");
  auto dx = at::empty_like(x);
  auto dwb = at::empty({2, C}, x.options().dtype(param_dtype));
  at::Tensor dres;
  if (want_dres) dres = at::empty_like(x);
  if (x.numel() == 0) {
    dwb.zero_();
    if (want_dres) return {dx, dwb[0], dwb[1], dres};
    return {dx, dwb[0], dwb[1]};
  }
  const at::Tensor wt = param_or(weight, x, C, true), bt = param_or(bias, x, C, false);
  auto stream = at::hip::getCurrentHIPStream();
  const auto fopt = x.options().dtype(at::kFloat);
  const bool streamed = g.chunks > 1;
  const int nb = (int)(N * g.chunks);
  auto part = at::empty({nb, 2 * C}, fopt);
  at::Tensor ws, csum;
  if (streamed) {
    ws = at::empty({N, g.chunks, G, 2}, fopt);
    csum = at::empty({N, G, 2}, fopt);
  }
  const dim3 grid((unsigned)(N * g.segs * g.chunks)), block(kGnThreads);
  auto run = [&](auto tag) {
    using T = decltype(tag);
    const T* dyp = reinterpret_cast<const T*>(dy.data_ptr());
    const T* xp = reinterpret_cast<const T*>(x.data_ptr());
    const T* yp = hy ? reinterpret_cast<const T*>(y->data_ptr()) : nullptr;
    T* dxp = reinterpret_cast<T*>(dx.data_ptr());
    T* drp = want_dres ? reinterpret_cast<T*>(dres.data_ptr()) : nullptr;
    const float *wp = wt.data_ptr<float>(), *bp = bt.data_ptr<float>();
    const float *mp = mean.data_ptr<float>(), *sp = rstd.data_ptr<float>();
    if (!streamed) {
      const BwdFn<T> k = small_slab(g, sizeof(T)) ? bwd_for<T, kResident, kGnSlabSmall>(g.cg)
                                                  : bwd_for<T, kResident, kGnSlab>(g.cg);
      hipLaunchKernelGGL(k, grid, block, 0, stream, dyp, xp, yp, wp, bp, mp, sp, g, (int)act, (float)clip, dxp,
                         drp, part.data_ptr<float>(), (float*)nullptr, (const float*)nullptr);
      return;
    }
    hipLaunchKernelGGL((bwd_for<T, kStats, 0>(g.cg)), grid, block, 0, stream, dyp, xp, yp, wp, bp, mp, sp, g,
                       (int)act, (float)clip, dxp, drp, part.data_ptr<float>(), ws.data_ptr<float>(),
                       (const float*)nullptr);
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3((unsigned)((N * G + 255) / 256)), dim3(256), 0, stream,
                       ws.data_ptr<float>(), N * G, g, csum.data_ptr<float>());
    hipLaunchKernelGGL((bwd_for<T, kApply, 0>(g.cg)), grid, block, 0, stream, dyp, xp, yp, wp, bp, mp, sp, g,
                       (int)act, (float)clip, dxp, (T*)nullptr, (float*)nullptr, (float*)nullptr,
                       (const float*)csum.data_ptr<float>());
  };
  if (x.scalar_type() == at::kBFloat16) run(__bf16{}); else run(float{});
  const int n2 = (int)(2 * C);
  if (param_dtype == at::kBFloat16)
    colreduce::launch(part.data_ptr<float>(), nb, n2, reinterpret_cast<__bf16*>(dwb.data_ptr()), stream);
  else
    colreduce::launch(part.data_ptr<float>(), nb, n2, dwb.data_ptr<float>(), stream);
  if (want_dres) return {dx, dwb[0], dwb[1], dres};
  return {dx, dwb[0], dwb[1]};
}

}  // namespace dmp
