// Large-tile MFMA bf16 TN GEMMs: the weight gradients dW = dy^T x of the
// transformer linears and of the wide convs (1x1, and k x k through the
// implicit-GEMM tap gather), and the Gram matrix of a strided sample.  The
// reduction dimension M = batch * positions is split across blocks into fp32
// partials that split_reduce_launch (conv/gemm_bf16.hip) sums.
//
// In this file:
//   gemm_tn_w4_kernel  4 waves, one per SIMD, 256 x 256 outputs (narrower
//                      TnShape tiles for sides of 64 / 128): the default
//   gemm_tn_pp_kernel  8 waves, ping-pong quadrant schedule: DMP_XL_PIPE=10
//                      and the gathers the 4-wave kernel does not take
// and their host dispatch (run_tn_pp).  The main-loop selection is the NT
// side's (gemm_xl.hip), read through get_gemm_xl_pipe(); what both sides use
// is in xl_common.h.
#include <algorithm>
#include <type_traits>
#include <ATen/hip/HIPContext.h>
#include "../api.h"
#include "../launch.h"
#include "xl_common.h"

namespace dmp {
namespace {

// ---------------------------------------------------------------------------
// Weight-gradient GEMM on the ping-pong schedule:
//   part[split][n][k] = sum_{m in split} A[m, n] * B[m, k]
// (A = dy [M, N], B = x [M, K] or the implicit-GEMM tap gather of an NHWC
// input).  The reduction runs over the huge M = batch*H*W, split across
// blocks; a column reduce sums the fp32 partials.  256 (n) x 256 (k) output
// tile, 8 waves as 2 x 4 (128 x 64 each), 64 m per K tile.  MFMA operands
// need 8 consecutive m per lane: the LDS holds m-major tiles and fragments
// come from ds_read_b64_tr_b16 (transposing read).  Each operand tile of a
// stage is 8 planes of [64 m][32 cols] (64-B rows, 32-B chunk XOR row & 1),
// so every 16 KB staging unit is 4 whole planes: U0 / U3 = the n columns of
// the waves' m-halves 0 / 1, U1 / U2 = the k columns of their n-halves 0 / 1.
// Quadrants run in the order (0,0) (0,1) (1,1) (1,0) as in gemm_xl_nt_kernel's
// PIPE 10; the unit schedule is the shallower one that kernel had in round 4
// (its removed PIPE 7): phase r of tile t stages U3(t+1), U1(t+1), U0(t+2),
// U2(t+2) (r = 0..3), so every unit is written >= 2 barrier slots after its
// previous contents were last read (WAR) and is retired by the vmcnt(4) of a
// phase >= 2 before its first reader (RAW).  LDS-DMA writes lane-linearly, so each lane fetches the
// logical 16 B that its physical slot holds under the swizzle.
// ---------------------------------------------------------------------------
struct TnPPArgs {
  const bf16* A; int64_t lda;
  const bf16* B; int64_t ldb;
  int M, N, K;
  int64_t rps;   // rows per split, a multiple of 64
  float* part;   // [splits][N][K]
  XlConv cv;     // cin > 0: B row m of a K tile = input pixel of its tap (K tile inside one tap)
  int gram = 0;  // 1: A = B = the gathered rows (Gram of a strided 1x1 sample; 4-wave kernel only)
};

// 32-B chunk XOR: row & 1 separates rows q, q+1 (one 256-B bank row holds 4
// rows); bit 3 separates rows r and r+8, which lanes l and l+16 of one
// ds_read_b64_tr_b16 half-wave read (they would otherwise share banks: 2x).
__device__ __forceinline__ int tn64_swz(int row) { return (row ^ (row >> 3)) & 1; }
__device__ __forceinline__ int tn64_off(int row, int col) {
  const int byte = col * 2;
  return row * 64 + ((((byte >> 5) ^ tn64_swz(row))) << 5) + (byte & 31);
}

__global__ __launch_bounds__(XTHREADS, 1) void gemm_tn_pp_kernel(const TnPPArgs p) {
  constexpr int PLANE = 64 * 64, OPER = 8 * PLANE;  // bytes
  __shared__ __attribute__((aligned(16))) char smem[4 * OPER];
  using v4i16 = short __attribute__((ext_vector_type(4)));
  using lds_v4 = __attribute__((address_space(3))) v4i16;
  const int M = p.M, N = p.N, K = p.K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int ntiles = (N + 255) >> 8, ktiles = (K + 255) >> 8;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile = bid % (ntiles * ktiles), split = bid / (ntiles * ktiles);
  const int n0 = (tile / ktiles) * 256, k0 = (tile % ktiles) * 256;
  const int64_t mb = (int64_t)split * p.rps;
  const int64_t me = min((int64_t)M, mb + p.rps);
  const int KT = (int)((me - mb + 63) >> 6);
  const XlConv cv = p.cv;
  const bool gather = cv.cin > 0;
  int tr = 0, tc = 0, kc0 = k0;
  if (gather) {
    const int tap = k0 / cv.cin;
    tr = tap / cv.kw;
    tc = tap - tr * cv.kw;
    kc0 = k0 - tap * cv.cin;
  }
  auto a_plane = [&](int buf, int pl) { return smem + buf * 2 * OPER + pl * PLANE; };
  auto b_plane = [&](int buf, int pl) { return smem + buf * 2 * OPER + OPER + pl * PLANE; };

  // staging roles: wave w writes blocks b = 2 (w & 1) + q (q = 0, 1) of the
  // unit's plane pi = w >> 1; lane -> physical row, 16-B slot
  const int pi = wave >> 1;
  int srow[2], scol[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int b = 2 * (wave & 1) + q;
    srow[q] = 16 * b + (lane >> 2);
    const int slot = lane & 3;
    scol[q] = ((((slot >> 1) ^ tn64_swz(srow[q]))) << 4) + (slot & 1) * 8;
  }
  auto stage_unit = [&](auto u, int kt) {
    constexpr int U = decltype(u)::value;
    const int buf = kt & 1;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t m = mb + (int64_t)kt * 64 + srow[q];
      char* dst;
      const bf16* src = g_zero_row;
      if constexpr (U == 0 || U == 3) {
        const int pl = (U == 0 ? 0 : 2) + (pi & 1) + (pi >> 1) * 4;  // {0,1,4,5} / {2,3,6,7}
        const int col = n0 + pl * 32 + scol[q];
        dst = a_plane(buf, pl) + ((2 * (wave & 1) + q) << 10);
        if (m < me && col < N) src = p.A + m * p.lda + col;
      } else {
        const int pl = 2 * pi + (U == 2 ? 1 : 0);                     // {0,2,4,6} / {1,3,5,7}
        const int col = pl * 32 + scol[q];
        dst = b_plane(buf, pl) + ((2 * (wave & 1) + q) << 10);
        if (m < me && k0 + col < K) {
          if (!gather) {
            src = p.B + m * p.ldb + k0 + col;
          } else {
            const int hw = cv.ho * cv.wo;
            const int mi = (int)m, n = mi / hw, r = mi - n * hw, oh = r / cv.wo, ow = r - oh * cv.wo;
            const int ih = oh * cv.stride - cv.pad + tr, iw = ow * cv.stride - cv.pad + tc;
            if ((unsigned)ih < (unsigned)cv.hi && (unsigned)iw < (unsigned)cv.wi)
              src = p.B + ((int64_t)(n * cv.hi + ih) * cv.wi + iw) * p.ldb + kc0 + col;
          }
        }
      }
      glds16(src, dst);
    }
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // tr-read lane roles (as gemm_tn_kernel): group g = lane >> 4 covers m rows
  // 8g..8g+7 of a k32 step; lane 4q+p of the group reads row q, cols 4p..4p+3
  const int g = lane >> 4, li = lane & 15, q4 = li >> 2, p4 = li & 3;
  bf16x8 qa[2][4], qb[2][2];
  auto tr_frag = [&](const char* plane, int ks, int col_in) {
    const int rb = ks * 32 + 8 * g + q4;
    v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(plane + tn64_off(rb, col_in)));
    v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(plane + tn64_off(rb + 4, col_in)));
    short __attribute__((ext_vector_type(8))) t8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, t8);
  };
  auto read_a = [&](int mq, int buf) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        qa[ks][i] = tr_frag(a_plane(buf, wr * 4 + mq * 2 + (i >> 1)), ks, (i & 1) * 16 + 4 * p4);
  };
  auto read_b = [&](int nq, int buf) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 2; ++j) qb[ks][j] = tr_frag(b_plane(buf, wc * 2 + nq), ks, j * 16 + 4 * p4);
  };
  auto quad = [&](auto mqc, auto nqc) {
    constexpr int MQ = decltype(mqc)::value, NQ = decltype(nqc)::value;
    barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[MQ * 4 + i][NQ * 2 + j] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[ks][i], qb[ks][j], acc[MQ * 4 + i][NQ * 2 + j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    barrier();
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  if (KT > 0) {
    stage_unit(I0{}, 0);
    stage_unit(I2{}, 0);
    stage_unit(I3{}, 0);
    stage_unit(I1{}, 0);
    if (KT > 1) {
      stage_unit(I0{}, 1);
      stage_unit(I2{}, 1);
      vmcnt<4>();
    } else {
      vmcnt<0>();
    }
    barrier();
    if (wr == 1) barrier();
    for (int kt = 0; kt < KT; ++kt) {
      const int buf = kt & 1;
      const bool n1 = kt + 1 < KT, n2 = kt + 2 < KT;
      read_a(0, buf);
      read_b(0, buf);
      if (n1) { stage_unit(I3{}, kt + 1); vmcnt<4>(); } else { vmcnt<0>(); }
      quad(I0{}, I0{});
      read_b(1, buf);
      if (n1) { stage_unit(I1{}, kt + 1); vmcnt<4>(); } else { vmcnt<0>(); }
      quad(I0{}, I1{});
      read_a(1, buf);
      if (n2) { stage_unit(I0{}, kt + 2); vmcnt<4>(); } else { vmcnt<0>(); }
      quad(I1{}, I1{});
      read_b(0, buf);
      if (n2) { stage_unit(I2{}, kt + 2); vmcnt<4>(); } else { vmcnt<0>(); }
      quad(I1{}, I0{});
    }
    if (wr == 0) barrier();
  }
  float* out = p.part + (int64_t)split * N * K;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + wc * 64 + j * 16 + (lane & 15);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = n0 + wr * 128 + i * 16 + (lane >> 4) * 4 + e;
        if (n < N && k < K) out[(int64_t)n * K + k] = acc[i][j][e];
      }
    }
}

// ---- 4-wave weight-gradient kernel (the TN form of gemm_xl_w4_kernel;
// profiles/README.md finding 70).  Same output tile, M split and fp32
// partials as gemm_tn_pp_kernel, but: one wave per SIMD computing 128 (n) x
// 128 (k) outputs in 256 AGPRs (inline-asm MFMAs, w4_mfma); LDS-DMA pieces of
// 8 m-rows x 128 B (full cache lines; the ping-pong kernel's 16 x 64 B pieces
// half-use 16 lines each) into [64 m][64 cols] planes whose 16-B chunk c of
// row r sits at c ^ tnw_swz(r) (conflict-free ds_read_b64_tr_b16: the 8 rows a
// half-wave reads -- 4 rows of each of two 16-lane groups, 8 apart -- land on
// all 64 banks); one barrier per 64-deep K tile:
//   S1: the k32-half-0 MFMAs, reading half 1's fragments of tile t;
//       vmcnt(0) + barrier (tile t + 1 landed, buffer t & 1 free);
//   S2: the half-1 MFMAs, copying tile t + 2 into buffer t & 1 (one copy per
//       4 MFMAs) and reading half 0 of tile t + 1.
// SRC: 0 = plain B rows, 2 = the implicit-GEMM tap gather of an NHWC input,
// 3 = both operands the gathered rows (the Gram of a strided 1x1 sample).
__device__ __forceinline__ int tnw_swz(int row) { return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2); }

// Narrow tiles (SRC 0 only): TNN x TNK = 64 x 256 / 256 x 64 (the four
// waves along the wide side, 64 x 64 each) or 128 x 256 / 256 x 128 (2 x 2
// waves, 64 x 128 / 128 x 64 each) for outputs with a side of 64 or 128
// (ResNet-50 layers 1-2: a 256 x 256 tile multiplied 2-16x the useful MFMA
// work there); the copies of the operand planes past the tile are skipped.
template <int TNN, int TNK>
struct TnShape {
  static constexpr int WGN = TNN == 64 ? 1 : TNK == 64 ? 4 : 2;  // wave grid along n / k
  static constexpr int WGK = 4 / WGN;
  static constexpr int MB = TNN / 16 / WGN, NB = TNK / 16 / WGK;  // 16-blocks per wave along n / k
};

template <int SRC, int TNN = 256, int TNK = 256>
__global__ __launch_bounds__(256, 1) void gemm_tn_w4_kernel(const TnPPArgs p) {
  static_assert(SRC == 0 || (TNN == 256 && TNK == 256), "narrow TN tiles: plain operands only");
  constexpr int PLANE = 64 * 128, OPER = 4 * PLANE, BUF = 2 * OPER;  // bytes
  using SH = TnShape<TNN, TNK>;
  constexpr int WGK = SH::WGK, MB = SH::MB, NB = SH::NB;
  static_assert(MB * 16 * SH::WGN == TNN && NB * 16 * WGK == TNK && (MB == 4 || MB == 8) && (NB == 4 || NB == 8),
                "TN tile shape");
  constexpr int NMF = MB * NB, NRD = MB + NB;  // MFMAs / fragment reads per wave and k32 half
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  using v4i16 = short __attribute__((ext_vector_type(4)));
  using lds_v4 = __attribute__((address_space(3))) v4i16;
  const int M = p.M, N = p.N, K = p.K;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WGK, wc = wave % WGK;
  // this wave's operand planes inside the tile (64 columns each): copies of the others are skipped
  const bool cpa = wave * 64 < TNN, cpb = wave * 64 < TNK;
  const int ntiles = (N + TNN - 1) / TNN, ktiles = (K + TNK - 1) / TNK;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile = bid % (ntiles * ktiles), split = bid / (ntiles * ktiles);
  const int n0 = (tile / ktiles) * TNN, k0 = (tile % ktiles) * TNK;
  const int64_t mb = (int64_t)split * p.rps;
  const int64_t me = min((int64_t)M, mb + p.rps);
  const int KT = (int)((me - mb + 63) >> 6);
  // SRC 2: the K tile (256 channels) lies inside one tap (Cin % 256 == 0)
  const XlConv cv = p.cv;
  int tr = 0, tc = 0, kc0 = k0;
  if constexpr (SRC >= 2) {
    const int tap = k0 / cv.cin;
    tr = tap / cv.kw;
    tc = tap - tr * cv.kw;
    kc0 = k0 - tap * cv.cin;
  }

  // copy c (0..15) of a K tile: operand c >> 3 (A = dy n columns, B = k
  // columns), plane `wave`, row group c & 7; lane L: row 8 (c & 7) + (L >> 3),
  // stored chunk L & 7, logical chunk (L & 7) ^ tnw_swz(row)
  const int prow = lane >> 3;
  const int lcol = wave * 64 + (((lane & 7) ^ tnw_swz(prow)) << 3);  // row & 15 = 8 (c & 1) + prow: bit 3 from c
  const int lcol8 = wave * 64 + (((lane & 7) ^ tnw_swz(8 + prow)) << 3);
  // buffer form (the global_load_lds form made the compiler drain every copy
  // before each k step's first ds_read): descriptors over THIS split's rows,
  // so a copy of a row past the split's end is out of range and lands as
  // zeros; columns past N / K read neighbouring bytes into outputs that are
  // never stored
  // The copies are inline asm: as compiler-visible LDS writes (either
  // builtin) they made it wait vmcnt(0) -- every copy in flight -- before
  // each transposing fragment read it cannot prove disjoint from them.  The
  // waits that order them (vmcnt, then the barrier) are explicit anyway.
  using i32x4 = int __attribute__((ext_vector_type(4)));
  const int64_t nrow = me - mb;
  auto desc = [&](const bf16* base, int64_t bytes) {
    const uint64_t a = reinterpret_cast<uint64_t>(base);
    i32x4 d;
    d[0] = __builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    d[1] = __builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));  // stride 0
    d[2] = __builtin_amdgcn_readfirstlane((int)min(bytes, (int64_t)0x7fffffff));
    d[3] = 0x00020000;
    return d;
  };
  // SRC 2: B's descriptor spans the whole NHWC input (a padding tap's offset
  // is past its end: the copy lands zeros); every lane tracks the output pixel
  // (n, oh, ow) of each of its 8 staged rows, advanced by 64 pixels per K tile
  // (no per-copy division: the divisions made this form spill)
  // (based at the split's first image: offsets stay 32-bit for inputs > 2 GB)
  const int64_t img = (int64_t)cv.hi * cv.wi * p.ldb;  // elements per image
  const int nbase = SRC >= 2 ? (int)(mb / max(1, cv.ho * cv.wo)) : 0;
  const int64_t bbytes = SRC >= 2 ? ((me - 1) / max(1, cv.ho * cv.wo) - nbase + 1) * img * 2 : nrow * p.ldb * 2;
  // SRC 3 (the Gram x_s^T x_s of a strided sample): A IS B, both gathered
  const i32x4 rsb = desc(SRC >= 2 ? p.B + nbase * img : p.B + mb * p.ldb, bbytes),
              rsa = SRC == 3 ? rsb : desc(p.A + mb * p.lda, nrow * p.lda * 2);
  const uint32_t oa0 = (uint32_t)((prow * p.lda + n0 + lcol) * 2), oa8 = (uint32_t)((prow * p.lda + n0 + lcol8) * 2);
  const uint32_t ob0 = (uint32_t)((prow * p.ldb + k0 + lcol) * 2), ob8 = (uint32_t)((prow * p.ldb + k0 + lcol8) * 2);
  int gn[8], goh[8], gow[8];
  const int hw = cv.ho * cv.wo, adv_oh = SRC >= 2 ? 64 / max(1, cv.wo) : 0, adv_ow = SRC >= 2 ? 64 % max(1, cv.wo) : 0;
  if constexpr (SRC >= 2) {
#pragma unroll
    for (int rg = 0; rg < 8; ++rg) {
      const int mi = (int)min(mb + 8 * rg + prow, (int64_t)M - 1), n = mi / hw, r = mi - n * hw;
      gn[rg] = n - nbase;
      goh[rg] = r / cv.wo;
      gow[rg] = r - goh[rg] * cv.wo;
    }
  }
  // SRC 2: the 8 B row offsets of K tile kt, then advance every row by 64 pixels
  uint32_t bo[8];
  auto gather_rows = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int rg = 0; rg < 8; ++rg) {
      const int ih = goh[rg] * cv.stride - cv.pad + tr, iw = gow[rg] * cv.stride - cv.pad + tc;
      const bool ok = kt * 64 + 8 * rg + prow < nrow && (unsigned)ih < (unsigned)cv.hi && (unsigned)iw < (unsigned)cv.wi;
      const int64_t pix = ((int64_t)gn[rg] * cv.hi + ih) * cv.wi + iw;
      bo[rg] = ok ? (uint32_t)((pix * p.ldb + kc0 + ((rg & 1) ? lcol8 : lcol)) * 2) : 0xfffffff0u;
      int ow = gow[rg] + adv_ow, oh = goh[rg] + adv_oh, n = gn[rg];
      if (ow >= cv.wo) { ow -= cv.wo; ++oh; }
#pragma unroll
      for (int w = 0; w < 3; ++w)  // adv_oh + 1 <= 3 ho (host-checked)
        if (oh >= cv.ho) { oh -= cv.ho; ++n; }
      gow[rg] = ow; goh[rg] = oh; gn[rg] = n;
    }
  };
  const uint32_t lds0 = (uint32_t)reinterpret_cast<uintptr_t>(smem);
  auto dma = [&](int kt, int buf, int c) __attribute__((always_inline)) {
    const int rg = c & 7;
    const bool odd = rg & 1;  // row bit 3
    const int ldst = __builtin_amdgcn_readfirstlane((int)(lds0 + buf * BUF + (c >> 3) * OPER + wave * PLANE + rg * 1024));
    uint32_t voff = c < 8 ? (odd ? oa8 : oa0) + (uint32_t)(8 * rg * p.lda * 2)
                          : (odd ? ob8 : ob0) + (uint32_t)(8 * rg * p.ldb * 2);
    int soff = __builtin_amdgcn_readfirstlane((int)(kt * 64 * (c < 8 ? p.lda : p.ldb) * 2));
    if constexpr (SRC == 2)
      if (c >= 8) {
        voff = bo[rg];
        soff = 0;
      }
    if constexpr (SRC == 3) {  // A's columns n0.. of the same gathered rows (a zero row stays zero)
      voff = c >= 8 || bo[rg] == 0xfffffff0u ? bo[rg] : bo[rg] + (uint32_t)((n0 - kc0) * 2);
      soff = 0;
    }
    unsigned keep;
    if ((c < 8 && !cpa) || (c >= 8 && !cpb)) return;  // a plane past a narrow tile
    if (c < 8)
      asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
                   "buffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "s"(ldst), "v"(voff), "s"(rsa), "s"(soff) : "memory");
    else
      asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
                   "buffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "s"(ldst), "v"(voff), "s"(rsb), "s"(soff) : "memory");
  };

  // tr-read lane roles (as gemm_tn_pp_kernel): group g = lane >> 4 covers m
  // rows 8g..8g+7 of a k32 step; lane 4q+p of the group reads row q (+4 for
  // the high half), cols 4p..4p+3 of the fragment's 16 columns
  const int g = lane >> 4, li = lane & 15, q4 = li >> 2, p4 = li & 3;
  auto tr_frag = [&](const char* plane, int h, int cin) __attribute__((always_inline)) {  // cin: column within the 64-col plane, % 16 == 0
    const int r0 = h * 32 + 8 * g + q4, r1 = r0 + 4;
    const int cb = (cin + 4 * p4) * 2;  // byte within the row
    const char* a0 = plane + r0 * 128 + ((((cb >> 4) ^ tnw_swz(r0))) << 4) + (cb & 15);
    const char* a1 = plane + r1 * 128 + ((((cb >> 4) ^ tnw_swz(r1))) << 4) + (cb & 15);
    v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)a0);
    v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)a1);
    short __attribute__((ext_vector_type(8))) t8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, t8);
  };
  bf16x8 ra[2][MB], rb[2][NB];
  // fragment read r (0..NRD-1) of k32 half H: A block (n) r == 0 ? 0 : r - NB, B blocks (k) 0..NB-1 for r = 1..NB
  auto rd = [&](auto hc, int buf, int r) __attribute__((always_inline)) {
    constexpr int H = decltype(hc)::value;
    const bool isb = r >= 1 && r <= NB;
    const int blk = r == 0 ? 0 : (isb ? r - 1 : r - NB);
    const int col = (isb ? wc * NB : wr * MB) * 16 + blk * 16;  // within the operand tile
    const char* plane = smem + buf * BUF + (isb ? OPER : 0) + (col >> 6) * PLANE;
    if (isb) rb[H][blk] = tr_frag(plane, H, col & 63);
    else ra[H][blk] = tr_frag(plane, H, col & 63);
  };
  f32x4 acc[MB][NB];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  // operands swapped: acc[i][j] holds the transposed 16 x 16 block: lane =
  // output row n (i), registers = 4 consecutive output columns k (j).
  // Read r follows MFMA (r NMF) / NRD, copy c MFMA (c NMF) / 16 (the 256 x 256
  // tile: one read / copy per 4 MFMAs); closed forms, so every index folds.
  auto iter = [&](auto st, auto rdn, int kt) __attribute__((always_inline)) {
    constexpr bool STAGE = decltype(st)::value, READ = decltype(rdn)::value;
    const int buf = kt & 1;
    if constexpr (SRC >= 2 && STAGE) gather_rows(kt + 2);
#pragma unroll
    for (int n = 0; n < NMF; ++n) {
      w4_mfma(acc[n / NB][n % NB], rb[0][n % NB], ra[0][n / NB]);
      const int r = (n * NRD + NMF - 1) / NMF;
      if (r < NRD && r * NMF / NRD == n) rd(I1{}, buf, r);
    }
    asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    barrier();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < NMF; ++n) {
      w4_mfma(acc[n / NB][n % NB], rb[1][n % NB], ra[1][n / NB]);
      if constexpr (STAGE) {
        const int c = (n * 16 + NMF - 1) / NMF;
        if (c < 16 && c * NMF / 16 == n) dma(kt + 2, buf, c);
      }
      if constexpr (READ)
        if ((n & 1) == 1 && (n >> 1) < NRD) rd(I0{}, buf ^ 1, n >> 1);
    }
  };
  if (KT > 0) {
    if constexpr (SRC >= 2) gather_rows(0);
#pragma unroll
    for (int c = 0; c < 16; ++c) dma(0, 0, c);
    if (KT > 1) {
      if constexpr (SRC >= 2) gather_rows(1);
#pragma unroll
      for (int c = 0; c < 16; ++c) dma(1, 1, c);
      // tile 0 landed: at most one tile of this wave's copies (16, 8 or 0) in flight
      if (cpa && cpb) vmcnt<16>();
      else if (cpa || cpb) vmcnt<8>();
      else vmcnt<0>();
    } else {
      vmcnt<0>();
    }
    barrier();
#pragma unroll
    for (int r = 0; r < NRD; ++r) rd(I0{}, 0, r);
    int kt = 0;
    for (; kt + 2 < KT; ++kt) iter(std::true_type{}, std::true_type{}, kt);
    if (kt + 1 < KT) iter(std::false_type{}, std::true_type{}, kt++);
    iter(std::false_type{}, std::false_type{}, kt);
    w4_drain();
  }
  // fp32 partials: lane = row n, 16-B pieces of 4 consecutive k
  float* out = p.part + (int64_t)split * N * K;
  const int lrow = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    const int n = n0 + wr * MB * 16 + i * 16 + lrow;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int k = k0 + wc * NB * 16 + j * 16 + lk * 4;
      if (n < N && k < K) *reinterpret_cast<f32x4*>(out + (int64_t)n * K + k) = acc[i][j];
    }
  }
}

// ---------------------------------------------------------------------------
// Host side: split choice, kernel selection, launches.
// ---------------------------------------------------------------------------
int g_tn_xl_rounds = 0;  // 0: auto; else rounds of 256 blocks (tools/tn_xl_bench.py sweeps)
int g_tn_narrow = 1;     // narrow TN tiles for sides of 64 / 128 (set_tn_narrow, A/B)

// rows per M split (a multiple of 64): one or two full rounds of 1-block/CU
// work, every split >= 16 K tiles
int64_t tn_rows_per_split(int M, int N, int K, int tnn = 256, int tnk = 256) {
  const int tiles = ((N + tnn - 1) / tnn) * ((K + tnk - 1) / tnk);
  const int mtl = (M + 63) / 64;
  int rounds = tiles >= 256 ? (tiles + 255) / 256 : (tiles * std::max(1, 256 / tiles) >= 192 ? 1 : 2);
  if (g_tn_xl_rounds > 0) rounds = g_tn_xl_rounds;
  const int splits = std::max(1, std::min(256 * rounds / tiles, mtl / 16));
  int64_t rps = ((int64_t)M + splits - 1) / splits;
  return (rps + 63) / 64 * 64;
}

// the gather form addresses the images one M split touches through 32-bit
// offsets from the split's first image (the kernel's descriptor base)
bool tn_w4_gather_fits(const TnPPArgs& a) {
  const int64_t hw = std::max(1, a.cv.ho * a.cv.wo);
  const int64_t imgs = std::min<int64_t>(a.M / hw + 1, a.rps / hw + 2);
  return (int64_t)a.cv.hi * a.cv.wi * imgs * a.ldb * 2 < ((int64_t)1 << 31) - 16;
}

at::Tensor run_tn_pp(TnPPArgs a, const at::Tensor& like, at::ScalarType out_dtype, at::Tensor acc = at::Tensor()) {
  const int M = a.M, N = a.N, K = a.K;
  auto out = acc.defined() ? acc : at::empty({N, K}, like.options().dtype(out_dtype));
  if (M == 0) return acc.defined() ? out : out.zero_();
  // plain operands on the 4-wave kernel: the narrowest tile that covers a
  // side of 64 / 128 (TnShape); the gather forms keep 256 x 256
  const int pipe = get_gemm_xl_pipe();
  const bool plain_w4 = pipe == 11 && a.cv.cin == 0;
  const int tnn = !plain_w4 || !g_tn_narrow ? 256 : N <= 64 ? 64 : K <= 64 ? 256 : N <= 128 ? 128 : 256;
  const int tnk = !plain_w4 || !g_tn_narrow || tnn != 256 ? 256 : K <= 64 ? 64 : K <= 128 ? 128 : 256;
  const int tiles = ((N + tnn - 1) / tnn) * ((K + tnk - 1) / tnk);
  const int64_t rps = tn_rows_per_split(M, N, K, tnn, tnk);
  const int splits = (int)(((int64_t)M + rps - 1) / rps);
  a.rps = rps;
  auto part = at::empty({splits, N, K}, like.options().dtype(at::kFloat));
  a.part = part.data_ptr<float>();
  hipStream_t s = at::hip::getCurrentHIPStream();
  // weight gradients on the 4-wave kernel (finding 70; DMP_XL_PIPE=10: the
  // ping-pong one), the tap gather included when its input fits 32-bit offsets
  const dim3 grid(tiles * splits);
  if (plain_w4 && tnn == 64)
    hipLaunchKernelGGL((gemm_tn_w4_kernel<0, 64, 256>), grid, dim3(256), 0, s, a);
  else if (plain_w4 && tnk == 64)
    hipLaunchKernelGGL((gemm_tn_w4_kernel<0, 256, 64>), grid, dim3(256), 0, s, a);
  else if (plain_w4 && tnn == 128)
    hipLaunchKernelGGL((gemm_tn_w4_kernel<0, 128, 256>), grid, dim3(256), 0, s, a);
  else if (plain_w4 && tnk == 128)
    hipLaunchKernelGGL((gemm_tn_w4_kernel<0, 256, 128>), grid, dim3(256), 0, s, a);
  else if (plain_w4)
    hipLaunchKernelGGL(gemm_tn_w4_kernel<0>, grid, dim3(256), 0, s, a);
  else if (a.gram)
    hipLaunchKernelGGL(gemm_tn_w4_kernel<3>, dim3(tiles * splits), dim3(256), 0, s, a);
  else if (pipe == 11 && (64 / a.cv.wo + 1) <= 3 * a.cv.ho && tn_w4_gather_fits(a))
    hipLaunchKernelGGL(gemm_tn_w4_kernel<2>, dim3(tiles * splits), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(gemm_tn_pp_kernel, dim3(tiles * splits), dim3(XTHREADS), 0, s, a);
  DMP_HIP_CHECK(hipGetLastError());
  split_reduce_launch(a.part, splits, (int64_t)N * K, out, s, acc.defined());
  return out;
}

}  // namespace

// dW = A^T B on the ping-pong TN kernel: A [M, N], B [M, K] bf16 row-major.
at::Tensor gemm_tn_xl(const at::Tensor& A, const at::Tensor& B, at::ScalarType out_dtype,
                      const c10::optional<at::Tensor>& out) {
  check_bf16_2d(A, "A");
  check_bf16_2d(B, "B");
  TORCH_CHECK(A.size(0) == B.size(0), "gemm_tn_xl: M mismatch");
  TORCH_CHECK(A.size(1) % 8 == 0 && B.size(1) % 8 == 0, "gemm_tn_xl: N, K must be multiples of 8");
  TORCH_CHECK(A.size(0) < (1LL << 31), "gemm_tn_xl: M out of range");
  TORCH_CHECK(out_dtype == at::kFloat || out_dtype == at::kBFloat16, "gemm_tn_xl: fp32 or bf16 output");
  TnPPArgs a{};
  a.A = reinterpret_cast<const bf16*>(A.data_ptr()); a.lda = A.stride(0);
  a.B = reinterpret_cast<const bf16*>(B.data_ptr()); a.ldb = B.stride(0);
  a.M = (int)A.size(0); a.N = (int)A.size(1); a.K = (int)B.size(1);
  return run_tn_pp(a, A, out_dtype, acc_target(out, (int64_t)a.N * a.K, out_dtype, "gemm_tn_xl"));
}

// Gram G = x_s^T x_s (fp32 [Cin, Cin]) of the stride-s sample x[:, :, ::s, ::s]
// of an NHWC input, both operands gathered in place by the 4-wave TN kernel
// (the folded downsample BN's statistics, ops/bn_fold.py).  Cin % 256 == 0.
at::Tensor gram_strided_xl(const at::Tensor& x, int64_t stride, int64_t ho, int64_t wo) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 4 &&
                  x.is_contiguous(at::MemoryFormat::ChannelsLast), "gram_strided_xl: x must be channels_last bf16");
  const int64_t nb = x.size(0), cin = x.size(1), hi = x.size(2), wi = x.size(3);
  TORCH_CHECK(cin % 256 == 0, "gram_strided_xl: Cin must be a multiple of 256");
  TORCH_CHECK(stride >= 1 && (ho - 1) * stride < hi && (wo - 1) * stride < wi, "gram_strided_xl: bad geometry");
  TORCH_CHECK(nb * ho * wo < (1LL << 31), "gram_strided_xl: too many pixels");
  TnPPArgs a{};
  a.A = a.B = reinterpret_cast<const bf16*>(x.data_ptr());
  a.lda = a.ldb = cin;
  a.M = (int)(nb * ho * wo); a.N = (int)cin; a.K = (int)cin;
  a.cv.cin = (int)cin; a.cv.hi = (int)hi; a.cv.wi = (int)wi; a.cv.ho = (int)ho; a.cv.wo = (int)wo;
  a.cv.stride = (int)stride; a.cv.pad = 0; a.cv.kw = 1;
  a.gram = 1;
  a.rps = tn_rows_per_split(a.M, a.N, a.K);
  TORCH_CHECK((64 / wo + 1) <= 3 * ho && tn_w4_gather_fits(a), "gram_strided_xl: geometry outside the 4-wave gather");
  return run_tn_pp(a, x, at::kFloat);
}

bool gram_strided_xl_supported(int64_t nb, int64_t cin, int64_t hi, int64_t wi, int64_t ho, int64_t wo) {
  if (cin % 256 != 0 || (64 / std::max<int64_t>(1, wo) + 1) > 3 * ho || nb * ho * wo >= (1LL << 31)) return false;
  TnPPArgs a{};
  a.M = (int)(nb * ho * wo); a.N = a.K = (int)cin; a.ldb = cin;
  a.cv.hi = (int)hi; a.cv.wi = (int)wi; a.cv.ho = (int)ho; a.cv.wo = (int)wo;
  a.rps = tn_rows_per_split(a.M, a.N, a.K);
  return tn_w4_gather_fits(a);
}

// Weight gradient of a kh x kw conv on the ping-pong TN kernel:
// dW[Cout, kh*kw*Cin] (tap-major) = dy^T @ im2col(x); dy [N*Ho*Wo, Cout]
// row-major, x NHWC (channels_last), Cin % 256 == 0 (a 256-wide K tile never
// straddles a tap).
at::Tensor conv_wgrad_xl(const at::Tensor& dy, const at::Tensor& x, int64_t kh, int64_t kw, int64_t stride,
                         int64_t pad, int64_t ho, int64_t wo, at::ScalarType out_dtype,
                         const c10::optional<at::Tensor>& out) {
  check_bf16_2d(dy, "dy");
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 4 &&
                  x.is_contiguous(at::MemoryFormat::ChannelsLast), "conv_wgrad_xl: x must be channels_last bf16");
  const int64_t nb = x.size(0), cin = x.size(1), hi = x.size(2), wi = x.size(3);
  TORCH_CHECK(cin % 256 == 0, "conv_wgrad_xl: Cin must be a multiple of 256");
  TORCH_CHECK(dy.size(0) == nb * ho * wo && dy.size(1) % 8 == 0, "conv_wgrad_xl: dy must be [N*Ho*Wo, Cout]");
  TORCH_CHECK(nb * hi * wi < (1LL << 31) && dy.size(0) < (1LL << 31), "conv_wgrad_xl: too many pixels");
  TORCH_CHECK(out_dtype == at::kFloat || out_dtype == at::kBFloat16, "conv_wgrad_xl: fp32 or bf16 output");
  TnPPArgs a{};
  a.A = reinterpret_cast<const bf16*>(dy.data_ptr()); a.lda = dy.stride(0);
  a.B = reinterpret_cast<const bf16*>(x.data_ptr()); a.ldb = cin;
  a.M = (int)dy.size(0); a.N = (int)dy.size(1); a.K = (int)(kh * kw * cin);
  a.cv.cin = (int)cin; a.cv.hi = (int)hi; a.cv.wi = (int)wi; a.cv.ho = (int)ho; a.cv.wo = (int)wo;
  a.cv.stride = (int)stride; a.cv.pad = (int)pad; a.cv.kw = (int)kw;
  return run_tn_pp(a, dy, out_dtype, acc_target(out, (int64_t)a.N * a.K, out_dtype, "conv_wgrad_xl"));
}

void set_tn_xl_rounds(int r) { g_tn_xl_rounds = r; }
void set_tn_narrow(bool on) { g_tn_narrow = on ? 1 : 0; }

}  // namespace dmp
