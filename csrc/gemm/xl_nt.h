// What the large-tile NT GEMM sources share: gemm_xl.hip (host side: policy,
// entry points, the route to a kernel) and the one-kernel files
// gemm_xl_nt8.hip (8 waves), gemm_xl_w4.hip (4 waves) and gemm_xl_x2.hip (two
// blocks per CU).  Internal to csrc/gemm.
//
//   C[M, N] = epi( A[M, K] * B[N, K]^T )        (both operands K-contiguous)
//
// Epilogues (what hipBLASLt + separate torch kernels would do in 2-3 passes):
//   XL_STORE     C = bf16(acc)
//   XL_BIAS      C = bf16(acc + b[n])
//   XL_BIAS_GELU Aux = bf16(acc + b[n]);  C = bf16(gelu(Aux))     (fc1 forward)
//   XL_DGELU     C = bf16(bf16(acc) * gelu'(Aux))                  (fc2 dgrad ->
//                the gradient at fc1's pre-activation: no GELU-backward pass)
//   XL_BIAS_RES  C = bf16(bf16(acc + b[n]) + R)                    (proj / fc2
//                forward + residual add)
//   XL_BIAS_RES_SCALE  C = bf16(fma(bf16(acc + b[n]), s[m / rows_per_sample], R))
//                (the same with a per-sample fp32 scale on the branch:
//                stochastic depth.  s == 1 gives XL_BIAS_RES's bits, s == 0 the
//                residual row)
// Rounding points match the unfused torch sequence (addmm -> bf16 -> gelu).
//
// The plain structs and enums are in dmp::xl: they stand in the launchers'
// signatures, which cross translation units.  The device helpers (xl_epilogue,
// shared by the 8-wave and the 4-wave kernel, among them) are in an unnamed
// namespace like xl_common.h's: one copy per source.
#pragma once

#include "xl_common.h"

namespace dmp {
namespace xl {

constexpr int XBM = 256;
constexpr int X2_BM = 256, X2_BN = 128;  // tile of gemm_x2_kernel (the host's use_x2 needs X2_BN)

enum XlEpi { XL_STORE = 0, XL_BIAS = 1, XL_BIAS_GELU = 2, XL_DGELU = 3, XL_BIAS_RES = 4,
             // conv epilogues (same semantics as gemm_bf16.hip's EPI_MOMENTS /
             // EPI_AFFINE "add" / EPI_BNBWD), for the wide 1x1 conv GEMMs
             XL_MOMENTS = 5, XL_ADD = 6, XL_BNBWD = 7,
             // C = act(acc * s[n] + t[n] (+ R)): conv + training-mode BN (+ residual)
             // + ReLU when the BN statistics were formed before the GEMM (ops/bn_fold.py)
             XL_AFFINE = 8,
             // XL_BNBWD with its operand set fixed at compile time (the runtime
             // flags cost the epilogue ~2x the VALU of the moments epilogue):
             // mask from y with x moments / mask from y, no x
             XL_BNBWD_Y = 9, XL_BNBWD_YO = 10,
             // XL_BIAS_RES with the branch scaled per sample (a linear epilogue
             // numbered after the conv ones: the existing values, and with them
             // every existing instantiation, stay as they were)
             XL_BIAS_RES_SCALE = 11 };
// the transformer-linear epilogues (two-buffer PIPE 0 form built, never on the
// two-blocks-per-CU conv kernel); the rest are the conv epilogues
__host__ __device__ constexpr bool is_linear_epi(int e) { return e < XL_MOMENTS || e == XL_BIAS_RES_SCALE; }
__host__ __device__ constexpr bool is_bnbwd(int e) { return e == XL_BNBWD || e == XL_BNBWD_Y || e == XL_BNBWD_YO; }

// Epilogues the 4-wave kernel takes.  The operand-heavy conv epilogues
// (folded-BN affine + residual, every BN-backward form) run on short-K 1x1
// GEMMs whose time is mostly epilogue, and with one wave per SIMD and half the
// threads per row pass their HBM round trips are less hidden: in the ResNet-50
// step XL_BNBWD_YO took 12.9 vs 10.8 ms and XL_AFFINE 10.4 vs 9.8 ms on the
// 4-wave kernel (profiles/README.md finding 69), so they keep the 8-wave
// ping-pong (PIPE 10).  XL_BNBWD's runtime operand flags would also spill
// accumulators behind the inline-asm MFMAs (tests/test_kernel_resources.py).
__host__ __device__ constexpr bool w4_epi(int e) { return e != XL_AFFINE && !is_bnbwd(e); }

// Output row map (XL_STORE only): GEMM row m = (n, oh, ow) of an ho x wo grid
// is written to row (n, s*oh + oy, s*ow + ox) of an hi x wi image -- one
// stride phase of a strided conv's data gradient.  s == 1: identity.
struct XlOutMap {
  int s = 1, ho = 1, wo = 1, hi = 1, wi = 1, oy = 0, ox = 0;
};

struct XlArgs {
  const bf16* A; int64_t lda;
  const bf16* B; int64_t ldb;
  bf16* C; int64_t ldc;
  int M, N, K;
  const bf16* bias;             // [N] (XL_BIAS*)
  bf16* aux; int64_t ldaux;     // XL_BIAS_GELU: pre-activation out; XL_DGELU: pre-activation in
  const bf16* R; int64_t ldr;   // XL_BIAS_RES / XL_ADD / XL_BNBWD residual (optional for BNBWD)
  int group_m;                  // tile-order group height (M tiles)
  float* part;                  // XL_MOMENTS / XL_BNBWD partials [2][mtiles][N]
  double* zsums;                // moments target to zero (common.h) or null
  const bf16* bx; int64_t ldbx; // XL_BNBWD: BN input x [M, N]
  const bf16* bny; int64_t ldby;// XL_BNBWD: BN output y [M, N] (mask source) or null
  const float *bmean, *binv, *bw, *bb;  // mask affine as in gemm_bf16.hip EPI_BNBWD
  CompactMap rmap;              // XL_BNBWD residual in compact stride-s form
  XlConv cv;                    // implicit-GEMM conv gather of A (PIPE 10 / 11)
  XlOutMap omap;                // C row map (XL_STORE)
  // second A source (plain GEMM): K columns k >= K1 come from A2[row, k - K1]
  // (the [dz | a] operand of a BN-folded data gradient); K1 % 64 == 0
  const bf16* A2; int64_t lda2; int K1;
  XlOutMap a2m;                 // A2 rows through a strided map (x_s of a folded downsample)
  const float* ebias;           // XL_BNBWD: per-column constant added to the GEMM output
  const float *esc, *esh;       // XL_AFFINE coefficients (null: 1 / 0)
  int erelu;                    // XL_AFFINE ReLU
  // rows per tile of the PIPE 10 kernel (0 = 256): 192..240 trims the tile so
  // that an MFMA-bound grid fills whole 1-block/CU rounds (pick_bm)
  int bm;
  // diagnostics (set_gemm_xl_trace): per block [entry, operands landed, main
  // loop done, epilogue done] in 10-ns ticks, HW_ID, XCC_ID; null = off
  unsigned long long* tdbg;
  // XL_BIAS_RES_SCALE: fp32 scale per sample [M / rows_per_sample]; row m
  // belongs to sample m / rows_per_sample (the T of a [B, T, D] activation)
  const float* rscale; int rows_per_sample;
};

// One launcher per kernel file: the switch from the runtime choice to that
// kernel's template instantiations.  A combination that was not built is an
// error naming it.  (The route to one of them: xl_launch in gemm_xl.hip.)
// gemm_xl_nt8.hip -- bn 128 | 256, pipe 0 | 1 | 10
void launch_xl_nt8(const XlArgs& a, int epi, int bn, int pipe, int blocks, hipStream_t s);
// gemm_xl_w4.hip -- epilogues with w4_epi; picks SRC from the operands and the tile shape from a.bm / a.N
void launch_xl_w4(const XlArgs& a, int epi, hipStream_t s);
// gemm_xl_x2.hip -- conv epilogues, N % X2_BN == 0
void launch_xl_x2(const XlArgs& a, int epi, hipStream_t s);

}  // namespace xl
using namespace xl;

namespace {

// Exact-GELU pieces for the epilogues: Phi(x) via erf(|x|/sqrt2) from
// Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7, far below the bf16 output's
// 2^-9 relative rounding) and phi(x) from the SAME exponential, since
// exp(-z^2) with z = x/sqrt2 is exp(-x^2/2).  ~12 VALU ops against erff's
// ~40: the epilogue runs after the MFMA loop at 1 block/CU, so its VALU time
// is not hidden (libm erff made the fused fc1 epilogue cost more than the
// separate GELU pass it replaces).
__device__ __forceinline__ void gelu_parts(float x, float& cdf, float& pdf) {
  const float z = fabsf(x) * 0.70710678118654752f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.f));
  const float e = __expf(-z * z);
  const float poly =
      fmaf(fmaf(fmaf(fmaf(1.061405429f, t, -1.453152027f), t, 1.421413741f), t, -0.284496736f), t, 0.254829592f) * t;
  const float erf_abs = fmaf(-poly, e, 1.f);
  cdf = 0.5f + 0.5f * copysignf(erf_abs, x);
  pdf = 0.39894228040143268f * e;
}
__device__ __forceinline__ float gelu_f(float x) {
  float c, d;
  gelu_parts(x, c, d);
  return x * c;
}
__device__ __forceinline__ float gelu_grad_f(float x) {
  float c, d;
  gelu_parts(x, c, d);
  return fmaf(x, d, c);
}

// 16-B chunk swizzle of a k32 region (rows of 64 B = 4 chunks, 4 rows per
// 256-B bank row).  ds_read_b128 is serviced in four 16-lane groups
// {0-3,12-15,20-27}, {4-11,16-19,28-31} and their +32 images
// (MI355X_MICROARCH.md §LDS); an MFMA fragment read has lane l on row l & 15,
// chunk l >> 4, so each group holds rows {0-3,12-15} of one chunk and rows
// 4-11 of the neighbouring chunk.  XOR-ing the chunk with g(row >> 2) for
// g = {0, 2, 3, 1} gives every group 16 distinct bank slots (a plain
// XOR with row >> 2 leaves 2-way conflicts: rows 0-3 and 4-7 collide).
__device__ __forceinline__ int chunk_xor(int q) { return (0x78 >> (2 * (q & 3))) & 3; }

// Tile order: bijective XCD remap (consecutive logical ids share an XCD and
// run concurrently), then groups of GM M-tiles walked column by column, so
// the ~32 tiles resident on one XCD form a GM x 32/GM patch whose A and B
// panels are both reused from that XCD's L2.
__device__ __forceinline__ void tile_coords(int nblocks, int mtiles, int ntiles, int gm_max,
                                            int& mt, int& nt) {
  const int bid = xcd_remap(blockIdx.x, nblocks);
  const int per_group = gm_max * ntiles;
  const int g = bid / per_group, r = bid - g * per_group;
  const int gm = min(gm_max, mtiles - g * gm_max);
  mt = g * gm_max + r % gm;
  nt = r / gm;
}

__device__ __forceinline__ int64_t xl_out_row(const XlOutMap& g, int row) {
  if (g.s == 1) return row;
  const int hw = g.ho * g.wo;
  const int n = row / hw, r = row - n * hw;
  const int oh = r / g.wo, ow = r - oh * g.wo;
  return ((int64_t)n * g.hi + oh * g.s + g.oy) * g.wi + ow * g.s + g.ox;
}

__device__ __forceinline__ void xl_mark(const XlArgs& p, int k) {
  if (p.tdbg && threadIdx.x == 0) p.tdbg[(int64_t)blockIdx.x * 8 + k] = __builtin_amdgcn_s_memrealtime();
}

// Epilogue of the NT kernels (8-wave and 4-wave):
// (acc [+ bias]) -> bf16 tile in LDS, then the row-contiguous pass with the
// fused operation; acc in the PIPE's register layout (10 / 11: transposed).
// PIPE 11 (gemm_xl_w4_kernel): 4 waves as 2 x 2, 128 x 128 outputs per wave,
// 256 threads in the row passes; every other PIPE: 8 waves as 2 x 4
__host__ __device__ constexpr int xl_waves(int pipe) { return pipe == 11 ? 4 : 8; }
template <int BN, int PIPE>
using XlAcc = f32x4[8][xl_waves(PIPE) == 4 ? BN / 32 : BN / 64];

// WMB (PIPE 11): 16-row blocks per wave actually computed (7: 224-row tile,
// wave row 1 starts at row 112; acc[7][*] unused).  WWN (PIPE 11): waves along
// N (1: four waves stacked along M over a BN = 128 tile)
template <int BN, int EPI, int PIPE, int LDS, int WMB = 8, int WWN = 2, typename ACC>
__device__ __forceinline__ void xl_epilogue(const XlArgs& p, ACC& acc, char* smem, int m0, int n0,
                                            int mt, int mtiles, int tbm = XBM) {
  constexpr int NW = xl_waves(PIPE), XTHREADS = NW * 64;
  constexpr int WTM = 16 * WMB, WTN = NW == 4 ? BN / WWN : BN / 4;
  constexpr int MI = WTM / 16, NI = WTN / 16;
  static_assert((WMB == 8 && WWN == 2) || PIPE == 11, "trimmed wave tiles: 4-wave kernel only");
  constexpr int CT_STRIDE = BN + 8;
  constexpr bool kMom = EPI == XL_MOMENTS || is_bnbwd(EPI) || EPI == XL_DGELU;
  // rows of this tile: [m0, min(M, m0 + tbm)); a trimmed tile's staged rows
  // past tbm belong to the next tile and are neither stored nor summed
  const int M = min(p.M, m0 + tbm), N = p.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = NW == 4 ? (WWN == 2 ? wave >> 1 : wave) : wave >> 2;
  const int wc = NW == 4 ? (WWN == 2 ? wave & 1 : 0) : wave & 3;
  (void)lane;
  // ---- batched epilogue operand loads (residual / BN input / BN output / aux).
  // Row passes of RPP rows; batch b covers passes [b PB, b PB + PB).  The
  // first batch goes out BEFORE the accumulator staging below and every later
  // batch one batch ahead of its use, so a whole tile's operand rows are in
  // flight through the epilogue instead of one batch at a time (finding 66:
  // the residual epilogue was ~10 us of an 18-20 us short-K tile, its two
  // batches each a full HBM round trip).
  constexpr int CV = BN / 8, RPP = XTHREADS / CV;
  const int cvi = tid % CV, rr0 = tid / CV;
  const int col = n0 + cvi * 8;
  constexpr bool kBatch = is_bnbwd(EPI) || EPI == XL_ADD || EPI == XL_AFFINE || EPI == XL_BIAS_RES ||
                          EPI == XL_DGELU || EPI == XL_BIAS_RES_SCALE;
  constexpr bool kL0 = kBatch;
  constexpr bool kL12 = is_bnbwd(EPI);
  constexpr bool kLx = EPI == XL_BNBWD || EPI == XL_BNBWD_Y, kLy = EPI == XL_BNBWD_Y || EPI == XL_BNBWD_YO;
  constexpr int NT = (kL0 ? 1 : 0) + (kLx ? 1 : 0) + (kLy ? 1 : 0);
  constexpr int NP = kBatch ? XBM / RPP : 0;
  constexpr int PB = NT >= 3 ? 2 : NT == 2 ? 4 : 8;  // two batches in flight: 2 PB NT 16-B loads per lane
  constexpr int NB = kBatch ? NP / PB : 1;
  // operand bases for branch-free loads: a missing operand reads a valid
  // dummy row (row 0 of C / of itself), its value is never used -- a
  // per-load branch would split every load into its own block, and the
  // compiler then waits for each one before the next (measured: the
  // forward affine epilogue kept exactly one load per lane in flight)
  const bf16* rsrc = EPI == XL_DGELU ? p.aux : p.R;  // GELU' reads the pre-activation
  const bf16* rbase = rsrc ? rsrc : p.C;
  const int64_t rld = rsrc ? (EPI == XL_DGELU ? p.ldaux : p.ldr) : 0;
  const bf16* xbase = p.bx ? p.bx : p.C;
  const int64_t xld = p.bx ? p.ldbx : 0;
  const bf16* ybase = p.bny ? p.bny : p.C;
  const int64_t yld = p.bny ? p.ldby : 0;
  // row pointers advance by a uniform RPP-row step (no per-row 64-bit
  // multiply); a row past M reads row 0 of the same operand instead
  // loads are issued by every lane (a load under a branch makes the compiler
  // drain the whole batch at the join): lanes past N read column N - 8
  const int coll = min(col, N - 8);
  const bf16* rrow = rbase + (int64_t)(m0 + rr0) * rld + coll;
  const int64_t rstep = (int64_t)RPP * rld;
  const bf16* xrow = xbase + (int64_t)(m0 + rr0) * xld + coll;
  const bf16* yrow = ybase + (int64_t)(m0 + rr0) * yld + coll;
  const int64_t xstep = (int64_t)RPP * xld, ystep = (int64_t)RPP * yld;
  bf16x8 L0[NB][PB], L1[NB][PB], L2[NB][PB];
  unsigned rok[NB];  // bit i: row pass b PB + i has a residual row (compact map)
  // XL_BIAS_RES_SCALE: the per-sample scale of each row pass, loaded with the
  // batch.  row / rows_per_sample without a divide per pass: q = hi32(row * mg)
  // with mg = floor((2^32 - 1) / d) is the quotient or one below it
  // (row * mg / 2^32 > row / d - 1 for row < 2^31), one compare-and-add fixes it
  constexpr bool kScale = EPI == XL_BIAS_RES_SCALE;
  float S0[NB][PB];
  const unsigned sdiv = kScale ? (unsigned)p.rows_per_sample : 1u;
  const unsigned smg = 0xffffffffu / sdiv;
  auto issue = [&](const int b) {
    rok[b] = 0;
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      const int pass = b * PB + i;
      const int row_u = m0 + rr0 + pass * RPP;
      const int row = min(row_u, M - 1);
      if constexpr (kL0) {
        const bf16x8* rp;
        if constexpr (is_bnbwd(EPI)) {
          int64_t rr = p.R ? compact_row(p.rmap, row) : -1;
          rok[b] |= (rr >= 0 ? 1u : 0u) << i;
          rr = rr >= 0 ? rr : 0;
          rp = reinterpret_cast<const bf16x8*>(rbase + rr * rld + coll);
        } else {
          rp = reinterpret_cast<const bf16x8*>(row_u < M ? rrow + pass * rstep : rbase + coll);
        }
        L0[b][i] = *rp;
      }
      if constexpr (kScale) {  // a row past M reads sample 0, as the residual reads row 0
        const unsigned r = row_u < M ? (unsigned)row_u : 0u;
        unsigned q = __umulhi(r, smg);
        q += (r - q * sdiv >= sdiv) ? 1u : 0u;
        S0[b][i] = p.rscale[q];
      }
      if constexpr (kL12) {
        if constexpr (kLx) L1[b][i] = *reinterpret_cast<const bf16x8*>(row_u < M ? xrow + pass * xstep : xbase + coll);
        if constexpr (kLy) L2[b][i] = *reinterpret_cast<const bf16x8*>(row_u < M ? yrow + pass * ystep : ybase + coll);
      }
    }
  };
  // BN-backward column constants, loaded ahead of everything else (branch-free:
  // an absent operand reads the zero row, a select picks the default)
  float bmu[8], bsc[8], bsh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bmu[j] = bsc[j] = bsh[j] = 0.f;
  if constexpr (is_bnbwd(EPI)) {
    const float* zf0 = reinterpret_cast<const float*>(g_zero_row);
    const f32x8 mu = *reinterpret_cast<const f32x8*>(p.bmean ? p.bmean + coll : zf0);
    f32x8 iv = {}, ww = {}, bb = {};
    if constexpr (EPI == XL_BNBWD) {
      iv = *reinterpret_cast<const f32x8*>(p.binv ? p.binv + coll : zf0);
      ww = *reinterpret_cast<const f32x8*>(p.bw ? p.bw + coll : zf0);
      bb = *reinterpret_cast<const f32x8*>(p.bb ? p.bb + coll : zf0);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bmu[j] = mu[j];
      if constexpr (EPI == XL_BNBWD) {
        bsc[j] = iv[j] * (p.bw ? ww[j] : 1.f);
        bsh[j] = bb[j] - bmu[j] * bsc[j];
      }
    }
  }
  bf16* ct = reinterpret_cast<bf16*>(smem);
  // per-column affine applied to the fp32 accumulator BEFORE the bf16 staging:
  // a bias / BN shift that nearly cancels acc (XL_BNBWD's folded-BN constant,
  // XL_AFFINE's -mean*scale) must not meet a bf16-rounded acc (finding 33)
  if constexpr (PIPE == 10 || PIPE == 11) {
    // transposed accumulators (see quad()): lane l holds row l & 15 and the 4
    // consecutive columns 4 (l >> 4) + e of each 16 x 16 block -> one 8-B LDS
    // write per block (a half-wave covers 16 rows x 16 B at a 528-B row pitch:
    // all 64 banks once) instead of four 2-B writes
    // the per-column coefficients first, then the first operand batch: a use
    // of a load waits for everything issued before it (in-order vmcnt), so
    // coefficients loaded after the batch would drain it before the staging
    // (branch-free as the batch: absent coefficients read the zero row,
    // columns past N read column N - 4, and selects pick the defaults)
    f32x4 s4a[NI], b4a[NI];
    const float* zf = reinterpret_cast<const float*>(g_zero_row);
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int colj = min(n0 + wc * WTN + j * 16 + (lane >> 4) * 4, N - 4);  // N % 8 == 0
      f32x4 s4 = {1.f, 1.f, 1.f, 1.f}, b4 = {0.f, 0.f, 0.f, 0.f};
      if constexpr (EPI == XL_BIAS || EPI == XL_BIAS_GELU || EPI == XL_BIAS_RES || EPI == XL_BIAS_RES_SCALE) {
#pragma unroll
        for (int e = 0; e < 4; ++e) b4[e] = (float)p.bias[colj + e];  // a bias view may be 2-B aligned only
      }
      if constexpr (is_bnbwd(EPI))
        b4 = *reinterpret_cast<const f32x4*>(p.ebias ? p.ebias + colj : zf);
      if constexpr (EPI == XL_AFFINE) {
        const f32x4 sl = *reinterpret_cast<const f32x4*>(p.esc ? p.esc + colj : zf);
        s4 = p.esc ? sl : s4;
        b4 = *reinterpret_cast<const f32x4*>(p.esh ? p.esh + colj : zf);
      }
      s4a[j] = s4;
      b4a[j] = b4;
    }
    __builtin_amdgcn_sched_barrier(0);  // keep the coefficient loads ahead of the batch
    // (4 waves: the 256 accumulators are still live here and the batch would
    // spill; it goes out after the staging instead)
    if constexpr (kBatch && NW == 8) issue(0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int lc = wc * WTN + j * 16 + (lane >> 4) * 4;
      const f32x4 s4 = s4a[j], b4 = b4a[j];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int row = wr * WTM + i * 16 + (lane & 15);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(acc[i][j][e], s4[e], b4[e]);
        *reinterpret_cast<bf16x4*>(ct + row * CT_STRIDE + lc) = __builtin_convertvector(v, bf16x4);
      }
    }
    if constexpr (kBatch && NW == 4) issue(0);
  } else {
  float bv[NI], sv[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int col = n0 + wc * WTN + j * 16 + (lane & 15);
    bv[j] = 0.f;
    sv[j] = 1.f;
    if constexpr (EPI == XL_BIAS || EPI == XL_BIAS_GELU || EPI == XL_BIAS_RES || EPI == XL_BIAS_RES_SCALE)
      bv[j] = col < N ? (float)p.bias[col] : 0.f;
    if constexpr (is_bnbwd(EPI))
      bv[j] = (col < N && p.ebias) ? p.ebias[col] : 0.f;
    if constexpr (EPI == XL_AFFINE) {
      sv[j] = (col < N && p.esc) ? p.esc[col] : 1.f;
      bv[j] = (col < N && p.esh) ? p.esh[col] : 0.f;
    }
  }
  if constexpr (kBatch) issue(0);
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int col = wc * WTN + j * 16 + (lane & 15);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = wr * WTM + i * 16 + (lane >> 4) * 4 + e;
        ct[row * CT_STRIDE + col] = (bf16)fmaf(acc[i][j][e], sv[j], bv[j]);
      }
    }
  }
  __syncthreads();
  float msum[8], msq[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { msum[j] = 0.f; msq[j] = 0.f; }
  if (col < N) {
    // Epilogue in batches of PB row passes (issued above / one batch ahead):
    // the loads must not sit behind the batch's stores -- C may alias them for
    // all the compiler knows, so a load-compute-store loop keeps ~2 loads per
    // lane in flight (measured 2.2-3.1 TB/s on the short-K conv epilogues at 1
    // block/CU, tools/epi_bench.py).  The load-free epilogues keep the
    // row-at-a-time loop below.
    bf16* const crow = p.C + (int64_t)(m0 + rr0) * p.ldc + col;
    const int64_t cstep = (int64_t)RPP * p.ldc;
    // XL_AFFINE without a residual still loads (a dummy row of C: branch-free
    // batch) and masks the bits to +0 instead of branching around the add
    const unsigned rmask = p.R ? 0xffffffffu : 0u;
    (void)rmask;
    if constexpr (kBatch) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b + 1 < NB) issue(b + 1);
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        const int lr = rr0 + (b * PB + i) * RPP;
        const int row = m0 + lr;
        if (row >= M) continue;
        bf16x8 v = *reinterpret_cast<const bf16x8*>(ct + lr * CT_STRIDE + cvi * 8);
        if constexpr (EPI == XL_MOMENTS) {
          const f32x8 f = __builtin_convertvector(v, f32x8);
#pragma unroll
          for (int j = 0; j < 8; ++j) { msum[j] += f[j]; msq[j] = fmaf(f[j], f[j], msq[j]); }
        } else if constexpr (EPI == XL_ADD || EPI == XL_BIAS_RES) {
          f32x8 f = __builtin_convertvector(v, f32x8);
          f += __builtin_convertvector(L0[b][i], f32x8);
          v = __builtin_convertvector(f, bf16x8);
        } else if constexpr (EPI == XL_BIAS_RES_SCALE) {  // one fma, one rounding
          f32x8 f = __builtin_convertvector(v, f32x8);
          const f32x8 r = __builtin_convertvector(L0[b][i], f32x8);
          const float sc = S0[b][i];
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = fmaf(f[j], sc, r[j]);
          v = __builtin_convertvector(f, bf16x8);
        } else if constexpr (EPI == XL_AFFINE) {  // v = bf16(acc * s + t) (staged)
          f32x8 f = __builtin_convertvector(v, f32x8);
          u32x4 rb = __builtin_bit_cast(u32x4, L0[b][i]);
          rb &= rmask;
          f += __builtin_convertvector(__builtin_bit_cast(bf16x8, rb), f32x8);
          if (p.erelu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = fmaxf(f[j], 0.f);
          }
          v = __builtin_convertvector(f, bf16x8);
        } else if constexpr (is_bnbwd(EPI)) {
          f32x8 g = __builtin_convertvector(v, f32x8);  // ebias already in (staging)
          if (p.R) {  // the other branch's gradient: summed in fp32, rounded once (as XL_ADD)
            if ((rok[b] >> i) & 1u) g += __builtin_convertvector(L0[b][i], f32x8);
            v = __builtin_convertvector(g, bf16x8);
            g = __builtin_convertvector(v, f32x8);
          }
          // bx null: BN input never materialised (ops/bn_fold.py) -- mask from y, sum dz only.
          // XL_BNBWD keeps the operand set a runtime choice (the x2 kernel's
          // contract); _Y / _YO fix it: mask from y, with / without x moments
          constexpr bool kY = EPI != XL_BNBWD, kX = EPI != XL_BNBWD_YO;
          f32x8 xv = {}, yv = {};
          if constexpr (kLx) xv = __builtin_convertvector(L1[b][i], f32x8);
          if constexpr (kLy) yv = __builtin_convertvector(L2[b][i], f32x8);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            // (xl_conv_run maps an operand set with y to _Y / _YO: plain
            // XL_BNBWD here always has x and no y)
            bool on;
            if constexpr (kY) on = yv[j] > 0.f;
            else on = fmaf(xv[j], bsc[j], bsh[j]) > 0.f;
            const float dz = on ? g[j] : 0.f;
            g[j] = dz;
            msum[j] += dz;
            if constexpr (kX) msq[j] = fmaf(dz, xv[j] - bmu[j], msq[j]);
          }
          v = __builtin_convertvector(g, bf16x8);
        } else if constexpr (EPI == XL_BIAS_GELU) {
          *reinterpret_cast<bf16x8*>(p.aux + (int64_t)row * p.ldaux + col) = v;
          f32x8 f = __builtin_convertvector(v, f32x8);
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = gelu_f(f[j]);
          v = __builtin_convertvector(f, bf16x8);
        } else if constexpr (EPI == XL_DGELU) {
          f32x8 f = __builtin_convertvector(v, f32x8);
          const f32x8 x = __builtin_convertvector(L0[b][i], f32x8);
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] *= gelu_grad_f(x[j]);
          v = __builtin_convertvector(f, bf16x8);
          const f32x8 fv = __builtin_convertvector(v, f32x8);  // the stored dh, as a column sum reads it
#pragma unroll
          for (int j = 0; j < 8; ++j) msum[j] += fv[j];
        }
        static_assert(!kBatch || EPI != XL_STORE, "batched epilogues write C rows unmapped");
        bf16x8* cp = reinterpret_cast<bf16x8*>(crow + (b * PB + i) * cstep);
        *cp = v;
      }
    }
    }
    if constexpr (!kBatch) {
#pragma unroll 8
      for (int pr = 0; pr < XBM / RPP; ++pr) {
        const int lr = rr0 + pr * RPP;
        const int row = m0 + lr;
        if (row >= M) continue;
        bf16x8 v = *reinterpret_cast<const bf16x8*>(ct + lr * CT_STRIDE + cvi * 8);
        if constexpr (EPI == XL_MOMENTS) {
          const f32x8 f = __builtin_convertvector(v, f32x8);
#pragma unroll
          for (int j = 0; j < 8; ++j) { msum[j] += f[j]; msq[j] = fmaf(f[j], f[j], msq[j]); }
        } else if constexpr (EPI == XL_BIAS_GELU) {
          *reinterpret_cast<bf16x8*>(p.aux + (int64_t)row * p.ldaux + col) = v;
          f32x8 f = __builtin_convertvector(v, f32x8);
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = gelu_f(f[j]);
          v = __builtin_convertvector(f, bf16x8);
        }
        const int64_t orow = EPI == XL_STORE ? xl_out_row(p.omap, row) : (int64_t)row;
        bf16x8* cp = reinterpret_cast<bf16x8*>(p.C + orow * p.ldc + col);
        *cp = v;
      }
    }
  }
  if (kMom && (EPI != XL_DGELU || p.part)) {
    // fold the RPP row groups of each column through LDS: one partial per M tile
    static_assert(2 * RPP * BN * 4 <= LDS, "moments scratch exceeds LDS");
    __syncthreads();  // every thread finished reading the C tile
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[(0 * RPP + rr0) * BN + cvi * 8 + j] = msum[j];
      red[(1 * RPP + rr0) * BN + cvi * 8 + j] = msq[j];
    }
    __syncthreads();
    for (int c = tid; c < BN; c += XTHREADS) {
      float s0 = 0.f, q0 = 0.f;
      for (int g = 0; g < RPP; ++g) {
        s0 += red[(0 * RPP + g) * BN + c];
        q0 += red[(1 * RPP + g) * BN + c];
      }
      if (n0 + c < N) {
        p.part[(int64_t)mt * N + n0 + c] = s0;
        p.part[(int64_t)(mtiles + mt) * N + n0 + c] = q0;
      }
    }
  }
}

}  // namespace
}  // namespace dmp
