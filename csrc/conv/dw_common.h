// Shared by the channels-last depthwise kernels (depthwise.hip: 3x3, a lane
// owns a 16-B channel vector; depthwise7.hip: 7x7, a lane owns a channel pair):
// the split of a 256-lane block over channels and work items with its size
// limits, the operand checks and the weight gradient's fp64 column reduce.
#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <algorithm>
#include <type_traits>
#include "../common.h"

namespace dmp {
namespace {

constexpr int kThreads = 256;

// Lane tid of a block serves channel unit blockIdx.y * tc + tid % tc and work
// item tid / tc of the block's pass; lanes with tid / tc >= spp are idle.
struct ChanSplit {
  int units;    // channel units: C / elements per lane
  int tc;       // channel units per block
  int spp;      // work items (strips, tiles) per block pass: kThreads / tc
  int cchunks;  // grid.y
};

inline ChanSplit chan_split(int64_t C, int per_lane) {
  ChanSplit s;
  s.units = (int)(C / per_lane);
  s.tc = std::min(s.units, kThreads);
  s.spp = kThreads / s.tc;
  s.cchunks = (s.units + s.tc - 1) / s.tc;
  return s;
}

// What the kernels' indices hold: int fields, int offsets within a row (W * C).
inline void check_sizes(int64_t N, int64_t C, int64_t H, int64_t W, int vec, const char* op) {
  TORCH_CHECK(N >= 1 && H >= 1 && W >= 1 && C >= vec && C % vec == 0, op,
              ": need N, H, W >= 1 and C a positive multiple of ", vec);
  TORCH_CHECK(N * H * W * C < (1LL << 40) && H < (1 << 20) && W * C < (1LL << 31), op, ": tensor too large");
}

// Block passes over `total` work items = grid.x of a one-pass-per-block launch.
inline int block_passes(int64_t total, const ChanSplit& s, const char* op) {
  const int64_t p = (total + s.spp - 1) / s.spp;
  TORCH_CHECK(p < (1LL << 31), op, ": grid too large");
  return (int)p;
}

// Weight gradient: about target_blocks blocks in all, each lane walking
// per_lane work items; one fp32 partial row per blockIdx.x.
struct WgradSplit {
  int per_lane, blocks;
};

inline WgradSplit wgrad_split(int passes, int cchunks, int target_blocks) {
  const int target = std::max(1, target_blocks / cchunks);
  WgradSplit s;
  s.per_lane = std::max(1, (passes + target - 1) / target);
  s.blocks = (passes + s.per_lane - 1) / s.per_lane;
  return s;
}

inline void check_nhwc(const at::Tensor& t, const char* name, bool allow_fp32) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 4, name, " must be a 4-D GPU tensor");
  const bool bf = t.scalar_type() == at::kBFloat16;
  TORCH_CHECK(bf || (allow_fp32 && t.scalar_type() == at::kFloat), name,
              allow_fp32 ? " must be bf16 or fp32" : " must be bf16");
  TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast), name, " must be channels-last");
  const int vec = bf ? 8 : 4;
  TORCH_CHECK(t.size(1) % vec == 0, name, ": channels must be a multiple of ", vec);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-B aligned");
}

// The weight as the kernels read it: [C][k*k] contiguous, bf16 or fp32, 16-B
// aligned -- the module's own [C,1,k,k] tensor when it already is (flat
// parameter views are padded to 8 elements), else one converted copy.
inline at::Tensor dw_weight(const at::Tensor& w, int64_t C, int k) {
  TORCH_CHECK(w.dim() == 4 && w.size(0) == C && w.size(1) == 1 && w.size(2) == k && w.size(3) == k,
              "depthwise weight must be [C,1,", k, ",", k, "] with the activation's C");
  TORCH_CHECK(w.is_cuda(), "depthwise weight must be a GPU tensor");
  if (w.is_contiguous() && (w.scalar_type() == at::kBFloat16 || w.scalar_type() == at::kFloat) &&
      reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0)
    return w;
  return w.to(at::kFloat).contiguous();
}

// f(__bf16{}) or f(float{}): the element type as the tag's type.
template <typename F>
void dispatch_bf16_f32(at::ScalarType dtype, F&& f) {
  TORCH_CHECK(dtype == at::kBFloat16 || dtype == at::kFloat, "expected bf16 or fp32");
  if (dtype == at::kBFloat16) f(__bf16{});
  else f(float{});
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// NE contiguous weight elements (one lane's channels x taps) by the widest
// word that divides the run: every lane's run starts at a multiple of its
// length from the 16-B aligned base, so it is aligned to that word.
template <typename WT, int NE>
__device__ __forceinline__ void load_run(const WT* __restrict__ p, WT (&e)[NE]) {
  constexpr int NB = NE * (int)sizeof(WT);
  using U = std::conditional_t<NB % 16 == 0, uint4, std::conditional_t<NB % 8 == 0, uint2, uint32_t>>;
  static_assert(NB % sizeof(U) == 0, "a weight run is a whole number of words");
  constexpr int NU = NB / (int)sizeof(U);
  const U* q = reinterpret_cast<const U*>(p);
  U r[NU];
#pragma unroll
  for (int i = 0; i < NU; ++i) r[i] = q[i];
  __builtin_memcpy(e, r, NB);
}

// Column j = t*C + c of the fp32 partial rows -> dw[c*kk + t] (t < kk) or
// db[c] (t == kk, only when the rows carry a bias column block); acc: added
// into the existing gradient.  fp64 accumulation, 32 row groups x 32 columns
// per block, folded by a fixed tree (no atomics).
template <typename OT>
__global__ __launch_bounds__(1024) void dw_colreduce_kernel(const float* __restrict__ part, int rows, int C, int kk,
                                                            OT* __restrict__ dw, OT* __restrict__ db, int acc) {
  const int ncol = (db != nullptr ? kk + 1 : kk) * C;
  const int cl = threadIdx.x % 32, g = threadIdx.x / 32;
  const int j = blockIdx.x * 32 + cl;
  double a = 0.0;
  if (j < ncol)
    for (int i = g; i < rows; i += 32) a += (double)part[(int64_t)i * ncol + j];
  __shared__ double l[1024];
  l[threadIdx.x] = a;
  __syncthreads();
  for (int s = 16; s > 0; s >>= 1) {
    if (g < s) l[threadIdx.x] += l[threadIdx.x + s * 32];
    __syncthreads();
  }
  if (g == 0 && j < ncol) {
    const int t = j / C, c = j % C;
    OT* o = t < kk ? dw + c * kk + t : db + c;
    *o = (OT)(acc ? l[threadIdx.x] + (double)(float)*o : l[threadIdx.x]);
  }
}

// dw [C,1,k,k] and db [C] (or undefined) share a dtype, bf16 or fp32.
inline void dw_colreduce_launch(const at::Tensor& part, int C, int kk, at::Tensor& dw, at::Tensor db, bool acc,
                                hipStream_t stream) {
  const int ncol = (db.defined() ? kk + 1 : kk) * C;
  TORCH_CHECK(part.size(1) == ncol && (!db.defined() || db.scalar_type() == dw.scalar_type()),
              "depthwise column reduce: partial rows or bias gradient do not match");
  dispatch_bf16_f32(dw.scalar_type(), [&](auto tag) {
    using OT = decltype(tag);
    hipLaunchKernelGGL((dw_colreduce_kernel<OT>), dim3((ncol + 31) / 32), dim3(1024), 0, stream,
                       part.data_ptr<float>(), (int)part.size(0), C, kk, reinterpret_cast<OT*>(dw.data_ptr()),
                       db.defined() ? reinterpret_cast<OT*>(db.data_ptr()) : nullptr, (int)acc);
  });
}

}  // namespace
}  // namespace dmp
