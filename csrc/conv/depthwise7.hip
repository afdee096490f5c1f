// Channels-last 7x7 depthwise convolution (groups == channels, stride 1,
// padding 3) -- forward (+ bias), data gradient (+ fused addend) and weight /
// bias gradient -- for the ConvNeXt blocks (models/convnext.py).
//
// Unlike the 3x3 (depthwise.hip, memory-bound) a 7x7 pass does 49 FMAs = 98
// FLOP per element against 4 B of compulsory bf16 traffic: 24.5 FLOP/B, above
// the machine balance of ~19.7 FLOP/B (fp32 vector peak / HBM), so the floor
// is the VALU and the inner loop has to be FMAs and little else.
//
// Design:
//   * a lane owns TWO channels (one 4-B bf16 pair; a wave covers 256
//     contiguous bytes of a pixel) and a tile of TH x TW = 4 x 8 outputs of one
//     image.  Its 49 taps x 2 channels of weights are 98 fp32 registers, the
//     tile's accumulators 64 more; all products are 2-wide (v_pk_fma_f32);
//   * the (TH+6) x (TW+6) input window is walked one input row at a time:
//     each of its 14 pairs is loaded once, converted to fp32 once and feeds
//     every output of the tile it touches (up to 4 rows x 7 columns) from
//     registers -- 140 loads per 1568 packed FMAs;
//   * loads go to clamped addresses and the out-of-image ones are zeroed by a
//     select on the raw 32-bit word (no branch, no per-tap address math); the
//     14 column offsets are computed once per tile;
//   * every tap / tile index in the unrolled loops is a compile-time constant:
//     nothing is runtime-indexed, scratch is 0;
//   * the weights are read in place from the module's [C,1,7,7] tensor (bf16
//     or fp32): a lane's two channels are 98 contiguous elements; the data
//     gradient is the same kernel with the taps read flipped;
//   * the weight gradient is the same loop nest with the roles swapped (the
//     tile's dy values live in registers -- a 2 x 8 tile here, the 100 sums
//     leave room for no more -- the 49 x 2 tap sums are the accumulators, the
//     bias gradient rides along as a 50th row); lanes of one
//     channel pair combine in LDS, a block writes one fp32 partial row and a
//     column reduce folds the rows in fp64 in a fixed order (no atomics).
#include "../api.h"
#include "dw_common.h"

namespace dmp {
namespace {

constexpr int TH = 4, TW = 8;       // outputs per lane: rows x columns (forward, data gradient)
constexpr int THW = 2;              // rows per lane of the weight gradient (its 100 sums leave room for 2 x 8 dy)
constexpr int K = 7, PAD = 3, KK = K * K;
constexpr int NCI = TW + K - 1;     // input columns of a tile's window
constexpr int kRows = KK + 1;       // weight-gradient partial rows: 49 taps + the bias gradient
constexpr int kWgradBlocks = 512;   // target block count of the weight gradient (partial rows)

using f32x2 = float __attribute__((ext_vector_type(2)));

struct Geo {
  int N, H, W, C;
  ChanSplit cs;  // units = channel pairs
  int th;        // tile height (TH, or THW for the weight gradient)
  int tiles_h, tiles_w;
  int64_t tiles;  // N * tiles_h * tiles_w
  int passes;     // block passes over the tiles: grid.x of the forward / data gradient
};

__device__ __forceinline__ f32x2 bf2_to_f32(uint32_t r) {
  f32x2 v;
  v.x = __uint_as_float(r << 16);
  v.y = __uint_as_float(r & 0xffff0000u);
  return v;
}

__device__ __forceinline__ uint32_t f32_to_bf2(f32x2 v) {
  using bf16x2 = __bf16 __attribute__((ext_vector_type(2)));
  const bf16x2 b = __builtin_convertvector(v, bf16x2);
  uint32_t r;
  __builtin_memcpy(&r, &b, 4);
  return r;
}

__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// The lane's 2 channels x 49 taps from the [C][49] weight: channels c0, c0+1
// are one contiguous run of 98 elements (4-B aligned for bf16, 8-B for fp32:
// c0 is even and the host checks the base).  FLIP reads tap 48 - t (the data
// gradient's rotated kernel).
template <typename WT, bool FLIP>
__device__ __forceinline__ void load_taps(const WT* __restrict__ wc, int c0, f32x2 (&wr)[KK]) {
  WT e[2 * KK];
  load_run(wc + (int64_t)c0 * KK, e);
#pragma unroll
  for (int t = 0; t < KK; ++t) {
    const int s = FLIP ? KK - 1 - t : t;
    wr[t].x = (float)e[s];
    wr[t].y = (float)e[KK + s];
  }
}

// A lane's place in the work split.
struct Lane {
  bool active;
  int c0;   // first of its two channels
  int n, oh0, ow0;
};

__device__ __forceinline__ Lane place(const Geo& g, int64_t tile, int lc, int ls) {
  Lane l;
  const int cpair = blockIdx.y * g.cs.tc + lc;
  l.active = ls < g.cs.spp && cpair < g.cs.units && tile < g.tiles;
  l.c0 = cpair * 2;
  const int tw = (int)(tile % g.tiles_w);
  const int64_t nr = tile / g.tiles_w;
  l.oh0 = (int)(nr % g.tiles_h) * g.th;
  l.n = (int)(nr / g.tiles_h);
  l.ow0 = tw * TW;
  return l;
}

// Column offsets (elements) of the 14 window columns, clamped into the row,
// and which of them are inside it.
__device__ __forceinline__ void window_cols(const Geo& g, int ow0, int (&off)[NCI], bool (&ok)[NCI]) {
#pragma unroll
  for (int ci = 0; ci < NCI; ++ci) {
    const int iw = ow0 - PAD + ci;
    ok[ci] = iw >= 0 && iw < g.W;
    off[ci] = clampi(iw, g.W - 1) * g.C;
  }
}

// Ties the next window row's load addresses (through `cw`) to an accumulator
// the current row has just updated.  The unrolled tile is one basic block, and
// without this the compiler moves every row's loads and conversions to its
// top (measured: 390 registers, or spills at 256); with it at most two rows
// are in flight.  Emits no instruction.
__device__ __forceinline__ void row_fence(int& cw, f32x2& a) {
  float t = a.x;
  asm volatile("" : "+v"(cw), "+v"(t));
  a.x = t;
}

// One window row: its 14 pairs from clamped addresses (always inside the
// tensor); the caller zeroes the out-of-image ones with a select.
__device__ __forceinline__ void load_row(const uint32_t* __restrict__ x, const Geo& g, int64_t img, int ih, int cw,
                                         const int (&off)[NCI], uint32_t (&raw)[NCI]) {
  const uint32_t* row = x + (((img + clampi(ih, g.H - 1)) * g.W) * g.C >> 1) + cw;
#pragma unroll
  for (int ci = 0; ci < NCI; ++ci) raw[ci] = row[off[ci] >> 1];
}

// ---------------------------------------------------------------------------
// forward (FLIP = false; extra = bias [C] in WT or null):
//   y[n,h,w,c] = b[c] + sum_{kh,kw} x[n,h+kh-3,w+kw-3,c] * w[c,kh,kw]
// data gradient (FLIP = true; extra = addend, bf16 of the output's shape, or null):
//   dx = add + the same stencil with w[c,6-kh,6-kw]
// grid.x = ceil(tiles / spp), grid.y = channel chunks
// ---------------------------------------------------------------------------
template <typename WT, bool FLIP>
__global__ __launch_bounds__(kThreads, 2) void dw7_kernel(const uint32_t* __restrict__ x,
                                                       const WT* __restrict__ wc,
                                                       const void* __restrict__ extra,
                                                       uint32_t* __restrict__ y, Geo g) {
  const int tid = threadIdx.x;
  const int lc = tid % g.cs.tc, ls = tid / g.cs.tc;
  const Lane l = place(g, (int64_t)blockIdx.x * g.cs.spp + ls, lc, ls);
  if (!l.active) return;
  f32x2 wr[KK];
  load_taps<WT, FLIP>(wc, l.c0, wr);
  f32x2 acc[TH][TW];
  f32x2 init = {0.f, 0.f};
  if (!FLIP && extra != nullptr) {
    const WT* b = reinterpret_cast<const WT*>(extra) + l.c0;
    init.x = (float)b[0];
    init.y = (float)b[1];
  }
#pragma unroll
  for (int o = 0; o < TH; ++o)
#pragma unroll
    for (int c = 0; c < TW; ++c) acc[o][c] = init;
  int off[NCI];
  bool ok[NCI];
  window_cols(g, l.ow0, off, ok);
  int cw = l.c0 >> 1;                             // 32-bit word of the channel pair
  const int64_t img = (int64_t)l.n * g.H;
  // row r+1 is in flight while row r is consumed (row_fence)
  constexpr int NR = TH + K - 1;  // input rows of the tile's window
  uint32_t raw[2][NCI];
  load_row(x, g, img, l.oh0 - PAD, cw, off, raw[0]);
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int ih = l.oh0 - PAD + r;
    const bool rok = ih >= 0 && ih < g.H;
    if (r + 1 < NR) load_row(x, g, img, ih + 1, cw, off, raw[(r + 1) & 1]);
#pragma unroll
    for (int ci = 0; ci < NCI; ++ci) {
      const f32x2 v = bf2_to_f32(rok && ok[ci] ? raw[r & 1][ci] : 0u);
#pragma unroll
      for (int o = 0; o < TH; ++o) {
        const int kh = r - o;
        if (kh < 0 || kh >= K) continue;
#pragma unroll
        for (int c = 0; c < TW; ++c) {
          const int kw = ci - c;
          if (kw < 0 || kw >= K) continue;
          acc[o][c] = fma2(v, wr[kh * K + kw], acc[o][c]);
        }
      }
    }
    row_fence(cw, acc[r < TH ? r : TH - 1][0]);
  }
  // The stores below are conditional (tile edges).  Pin the finished sums
  // here: otherwise each output's whole 49-FMA chain is sunk into its store's
  // branch and the entire converted window (224 registers) stays live to the end.
#pragma unroll
  for (int o = 0; o < TH; ++o)
#pragma unroll
    for (int c = 0; c < TW; ++c) asm volatile("" : "+v"(acc[o][c]));
  // The addend's 32 pairs are loaded up front from clamped addresses (and
  // pinned, as above): under the stores' branches each load was waited for
  // before the next was issued and the pass took twice as long.
  const uint32_t* add = FLIP ? reinterpret_cast<const uint32_t*>(extra) : nullptr;
  uint32_t araw[TH][TW];
  if (FLIP && add != nullptr) {
#pragma unroll
    for (int o = 0; o < TH; ++o) {
      const uint32_t* arow = add + (((img + min(l.oh0 + o, g.H - 1)) * g.W) * g.C >> 1) + cw;
#pragma unroll
      for (int c = 0; c < TW; ++c) araw[o][c] = arow[off[PAD + c] >> 1];
    }
#pragma unroll
    for (int o = 0; o < TH; ++o)
#pragma unroll
      for (int c = 0; c < TW; ++c) {
        asm volatile("" : "+v"(araw[o][c]));
        acc[o][c] += bf2_to_f32(araw[o][c]);  // fp32 add, one rounding in the store
      }
  }
#pragma unroll
  for (int o = 0; o < TH; ++o) {
    const int oh = l.oh0 + o;
    if (oh >= g.H) break;
    const int64_t rowoff = (((img + oh) * g.W) * g.C >> 1) + cw;
#pragma unroll
    for (int c = 0; c < TW; ++c) {
      const int ow = l.ow0 + c;
      if (ow >= g.W) break;
      y[rowoff + ((int64_t)ow * g.C >> 1)] = f32_to_bf2(acc[o][c]);
    }
  }
}

// ---------------------------------------------------------------------------
// weight / bias gradient partials: part[block][t*C + c], t < 49 the taps
//   dw[c,kh,kw] = sum dy[n,h,w,c] * x[n,h+kh-3,w+kw-3,c]
// and t = 49 the bias gradient sum dy.  Each lane walks tiles_per_lane tiles.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads, 2) void dw7_wgrad_kernel(const uint32_t* __restrict__ dy,
                                                             const uint32_t* __restrict__ x, Geo g,
                                                             int tiles_per_lane,
                                                             float* __restrict__ part) {
  const int tid = threadIdx.x;
  const int lc = tid % g.cs.tc, ls = tid / g.cs.tc;
  f32x2 acc[kRows];
#pragma unroll
  for (int t = 0; t < kRows; ++t) acc[t] = f32x2{0.f, 0.f};
  for (int k = 0; k < tiles_per_lane; ++k) {
    const Lane l = place(g, ((int64_t)blockIdx.x * tiles_per_lane + k) * g.cs.spp + ls, lc, ls);
    if (!l.active) break;
    int cw = l.c0 >> 1;
    const int64_t img = (int64_t)l.n * g.H;
    int off[NCI];
    bool ok[NCI];
    window_cols(g, l.ow0, off, ok);
    // the tile's dy: window columns PAD .. PAD+TW-1 are the output columns
    f32x2 gv[THW][TW];
    {
      uint32_t graw[THW][TW];
#pragma unroll
      for (int o = 0; o < THW; ++o) {
        const uint32_t* grow = dy + (((img + min(l.oh0 + o, g.H - 1)) * g.W) * g.C >> 1) + cw;
#pragma unroll
        for (int c = 0; c < TW; ++c) graw[o][c] = grow[off[PAD + c] >> 1];
      }
#pragma unroll
      for (int o = 0; o < THW; ++o)
#pragma unroll
        for (int c = 0; c < TW; ++c) {
          gv[o][c] = bf2_to_f32(l.oh0 + o < g.H && ok[PAD + c] ? graw[o][c] : 0u);
          acc[KK] += gv[o][c];
        }
    }
    constexpr int NR = THW + K - 1;
    uint32_t raw[2][NCI];
    load_row(x, g, img, l.oh0 - PAD, cw, off, raw[0]);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int ih = l.oh0 - PAD + r;
      const bool rok = ih >= 0 && ih < g.H;
      if (r + 1 < NR) load_row(x, g, img, ih + 1, cw, off, raw[(r + 1) & 1]);
#pragma unroll
      for (int ci = 0; ci < NCI; ++ci) {
        const f32x2 v = bf2_to_f32(rok && ok[ci] ? raw[r & 1][ci] : 0u);
#pragma unroll
        for (int o = 0; o < THW; ++o) {
          const int kh = r - o;
          if (kh < 0 || kh >= K) continue;
#pragma unroll
          for (int c = 0; c < TW; ++c) {
            const int kw = ci - c;
            if (kw < 0 || kw >= K) continue;
            acc[kh * K + kw] = fma2(v, gv[o][c], acc[kh * K + kw]);
          }
        }
      }
      row_fence(cw, acc[(r < K ? r : K - 1) * K]);
    }
  }
  // lanes of one channel pair (ls = 0 .. spp-1) combine in LDS, in a fixed order
  __shared__ float lds[2][kThreads];
#pragma unroll
  for (int t = 0; t < kRows; ++t) {
    lds[0][tid] = acc[t].x;
    lds[1][tid] = acc[t].y;
    __syncthreads();
    const int cpair = blockIdx.y * g.cs.tc + lc;
    if (ls == 0 && cpair < g.cs.units) {
      float s[2] = {0.f, 0.f};
      for (int r = 0; r < g.cs.spp; ++r) {
        s[0] += lds[0][r * g.cs.tc + lc];
        s[1] += lds[1][r * g.cs.tc + lc];
      }
      float2* dst = reinterpret_cast<float2*>(part + ((int64_t)blockIdx.x * kRows + t) * g.C + cpair * 2);
      *dst = make_float2(s[0], s[1]);
    }
    __syncthreads();
  }
}

Geo make_geo(int64_t N, int64_t C, int64_t H, int64_t W, int th) {
  check_sizes(N, C, H, W, 8, "dwconv7x7");
  Geo g;
  g.cs = chan_split(C, 2);
  g.N = (int)N;
  g.C = (int)C;
  g.H = (int)H;
  g.W = (int)W;
  g.th = th;
  g.tiles_h = (g.H + th - 1) / th;
  g.tiles_w = (g.W + TW - 1) / TW;
  g.tiles = (int64_t)g.N * g.tiles_h * g.tiles_w;
  g.passes = block_passes(g.tiles, g.cs, "dwconv7x7");
  return g;
}

template <bool FLIP>
at::Tensor run(const at::Tensor& x, const at::Tensor& w, const void* extra, const at::Tensor& wt) {
  const Geo g = make_geo(x.size(0), x.size(1), x.size(2), x.size(3), TH);
  auto y = at::empty_like(x, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto stream = at::hip::getCurrentHIPStream();
  dispatch_bf16_f32(wt.scalar_type(), [&](auto wtag) {
    using WT = decltype(wtag);
    hipLaunchKernelGGL((dw7_kernel<WT, FLIP>), dim3((unsigned)g.passes, (unsigned)g.cs.cchunks), dim3(kThreads), 0,
                       stream, reinterpret_cast<const uint32_t*>(x.data_ptr()),
                       reinterpret_cast<const WT*>(wt.data_ptr()), extra, reinterpret_cast<uint32_t*>(y.data_ptr()), g);
  });
  return y;
}

}  // namespace

at::Tensor dwconv7x7_forward(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias) {
  check_nhwc(x, "x", false);
  const auto wt = dw_weight(w, x.size(1), K);
  at::Tensor b;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->is_cuda() && bias->dim() == 1 && bias->size(0) == x.size(1), "dwconv7x7: bias must be [C]");
    // read in place when it has the taps' dtype (the module's usual case)
    b = bias->scalar_type() == wt.scalar_type() && bias->is_contiguous() ? *bias : bias->to(wt.scalar_type()).contiguous();
  }
  return run<false>(x, w, b.defined() ? b.data_ptr() : nullptr, wt);
}

at::Tensor dwconv7x7_dgrad(const at::Tensor& dy, const at::Tensor& w, const c10::optional<at::Tensor>& add) {
  check_nhwc(dy, "dy", false);
  const auto wt = dw_weight(w, dy.size(1), K);
  const void* ap = nullptr;
  if (add.has_value() && add->defined()) {
    check_nhwc(*add, "add", false);
    TORCH_CHECK(add->sizes() == dy.sizes(), "dwconv7x7_dgrad: add must have dx's shape");
    ap = add->data_ptr();
  }
  return run<true>(dy, w, ap, wt);
}

std::vector<at::Tensor> dwconv7x7_wgrad(const at::Tensor& dy, const at::Tensor& x, at::ScalarType w_dtype) {
  check_nhwc(dy, "dy", false);
  check_nhwc(x, "x", false);
  TORCH_CHECK(dy.sizes() == x.sizes(), "dwconv7x7_wgrad: dy / x shape mismatch");
  TORCH_CHECK(w_dtype == at::kBFloat16 || w_dtype == at::kFloat, "dwconv7x7_wgrad: weight gradient must be bf16 or fp32");
  const Geo g = make_geo(x.size(0), x.size(1), x.size(2), x.size(3), THW);
  const WgradSplit s = wgrad_split(g.passes, g.cs.cchunks, kWgradBlocks);
  auto stream = at::hip::getCurrentHIPStream();
  auto part = at::empty({(int64_t)s.blocks, (int64_t)kRows * g.C}, x.options().dtype(at::kFloat));
  hipLaunchKernelGGL(dw7_wgrad_kernel, dim3((unsigned)s.blocks, (unsigned)g.cs.cchunks), dim3(kThreads), 0, stream,
                     reinterpret_cast<const uint32_t*>(dy.data_ptr()), reinterpret_cast<const uint32_t*>(x.data_ptr()),
                     g, s.per_lane, part.data_ptr<float>());
  auto dw = at::empty({(int64_t)g.C, 1, K, K}, x.options().dtype(w_dtype));
  auto db = at::empty({(int64_t)g.C}, x.options().dtype(w_dtype));
  dw_colreduce_launch(part, g.C, KK, dw, db, false, stream);
  return {dw, db};
}

// The host's work split as plain integers (tests place shapes on its edges).
std::map<std::string, int64_t> dwconv7x7_plan(int64_t N, int64_t C, int64_t H, int64_t W) {
  const Geo g = make_geo(N, C, H, W, TH), gw = make_geo(N, C, H, W, THW);
  const WgradSplit s = wgrad_split(gw.passes, gw.cs.cchunks, kWgradBlocks);
  std::map<std::string, int64_t> d;
  d["tile_h"] = TH;
  d["tile_w"] = TW;
  d["threads"] = kThreads;
  d["channels_per_lane"] = 2;
  d["channels_per_block"] = g.cs.tc * 2;
  d["tiles_per_block"] = g.cs.spp;
  d["tiles_h"] = g.tiles_h;
  d["tiles_w"] = g.tiles_w;
  d["tiles"] = g.tiles;
  d["grid_x"] = g.passes;
  d["grid_y"] = g.cs.cchunks;
  d["wgrad_tile_h"] = THW;
  d["wgrad_tiles"] = gw.tiles;
  d["wgrad_tiles_per_lane"] = s.per_lane;
  d["wgrad_blocks"] = s.blocks;
  d["wgrad_rows"] = kRows;
  return d;
}

}  // namespace dmp
