// gemm_xl_w4_kernel: the 4-wave large-tile NT GEMM (PIPE 11, the default main
// loop of the 256-wide tiles): 256 x 256, 224 x 256 and 256 x 128 tiles.
// Epilogues, arguments and xl_epilogue: xl_nt.h; the host side that routes
// launches here: gemm_xl.hip.
#include <type_traits>
#include "xl_nt.h"

namespace dmp {
namespace {

// ---- PIPE 11: 4-wave 256 x 256 kernel (cdna_hip_programming.md §5; profiles/
// README.md finding 69).  One wave per SIMD computes 128 x 128 outputs (64
// accumulators, all 256 AGPRs, tied in-place MFMAs: w4_mfma), so each
// fragment read from LDS feeds 8 MFMAs (128 KB of fragment reads per CU and K
// tile, against 224 KB for the 8-wave 128 x 64 wave tiles) and the only
// synchronisation is one barrier per K tile.  Every LDS-DMA instruction copies
// 8 rows x 128 B -- one whole K tile of 8 rows, 8 full cache lines -- into an
// [256 rows][128 B] image with 16-B chunk c of row r at c ^ ((r >> 1) & 7)
// (conflict-free fragment reads).  Copies of half-line pieces (16 rows x 64 B)
// cost the MFMA issue stream ~25 % at 8192^3; full lines, one per 4 MFMAs
// spread over the copy segment, brought it from 1.39 to 1.54 PF/s.
//   S1: k-half 0 MFMAs, reading k-half 1's fragments of tile t (one ds_read
//       per 4 MFMAs); vmcnt(0) + barrier: tile t + 1 has landed, buffer t & 1
//       is free;
//   S2: k-half 1 MFMAs, copying tile t + 2 into buffer t & 1 (one per 4
//       MFMAs) and reading k-half 0 of tile t + 1 (first half of the segment).
// Operand staging features: plain A / B, the second A source (A2 from column
// K1, a strided row map), the conv tap gather (cv; zero taps from g_zero_row).
// (w4_mfma / w4_drain: xl_common.h, shared with the 4-wave TN kernel.)
__device__ __forceinline__ int w4_swz(int c, int row) { return c ^ ((row >> 1) & 7); }

// SRC (compile-time, so the copy stream between the MFMAs has no branches):
// 0 = plain A, by buffer_load ... lds with one 32-bit lane offset per piece
// (operands < 2 GB); 1 = plain A with the second source A2 from column K1;
// 2 = conv tap gather (global_load_lds, zero taps read g_zero_row)
// MB: 16-row MFMA blocks per wave (8: 256-row tiles; 7: 224-row tiles, which
// fill the last 1-block/CU round of grids such as ViT's N = 768 GEMMs, 591 ->
// 678 tiles in the same three rounds of 7/8 the work each: pick_bm).
// WN: waves along N (2: 2 x 2 waves, 256-wide tiles; 1: the four waves stacked
// along M with 64 x 128 each, a 256 x 128 tile for N = 128 -- ResNet-50's
// layer-2 stride-2 3x3 forward, which a 256-wide tile would half waste).
// NBW: 16-column blocks per wave (8; 4 with WN = 1 gives a 256 x 64 tile: for
// ResNet-50 layer 1's N = 64 conv1 forward and conv3 data gradient + BN
// backward it measured slower than gemm_nt's 256 x 64 tile in-step, 112.48
// vs 111.23 ms, finding 78, so no launch uses it).
template <int EPI, int SRC, int MB = 8, int WN = 2, int NBW = 8>
__global__ __launch_bounds__(256, 1) void gemm_xl_w4_kernel(const XlArgs p) {
  static_assert((WN == 2 && (MB == 8 || MB == 7) && NBW == 8) || (WN == 1 && MB == 4 && (NBW == 8 || NBW == 4)),
                "4-wave tile shapes");
  constexpr int TBM = (4 / WN) * 16 * MB, TBN = 16 * NBW * WN;  // tile rows / columns
  constexpr int NRD = NBW + MB, NMF = NBW * MB;  // fragment reads / MFMAs per wave and k-half
  constexpr int OPB = 256 * 128, BUF = 2 * OPB;  // one operand's K tile, one buffer (A | B)
  constexpr int EPI_LDS = XBM * (256 + 8) * 2;
  constexpr int LDS = 2 * BUF > EPI_LDS ? 2 * BUF : EPI_LDS;
  __shared__ __attribute__((aligned(16))) char smem[LDS];
  constexpr bool kMom = EPI == XL_MOMENTS || is_bnbwd(EPI) || EPI == XL_DGELU;
  if constexpr (kMom) zero_moments(p.zsums, 2 * p.N);
  const int M = p.M, N = p.N, K = p.K;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = WN == 2 ? wave >> 1 : wave, wc = WN == 2 ? wave & 1 : 0;
  const int mtiles = (M + TBM - 1) / TBM, ntiles = (N + TBN - 1) / TBN;
  int mt, nt;
  tile_coords(mtiles * ntiles, mtiles, ntiles, p.group_m, mt, nt);
  const int m0 = mt * TBM, n0 = nt * TBN;
  const int ktiles = K / XBK;

  // (a 224-row tile still stages 256 A rows: the last 32 are the next tile's,
  // read but never multiplied)
  // copy c (0..15) of a K tile: operand c >> 3 (A, B), 8-row piece
  // 8 wave + (c & 7); lane L: row 8 piece + (L >> 3), stored chunk L & 7,
  // logical chunk w4_swz(L & 7, row)
  const int lrow8 = lane >> 3;
  const int64_t abytes = ((int64_t)(M - 1) * p.lda + K) * 2, bbytes = ((int64_t)(N - 1) * p.ldb + K) * 2;
  const auto rsa = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, (short)0, (int)min(abytes, (int64_t)0x7fffffff),
                                                     0x00020000);
  const auto rsb = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, (short)0, (int)min(bbytes, (int64_t)0x7fffffff),
                                                     0x00020000);
  uint32_t oa[8], ob[8];
  const bf16* pa2[8];
  const XlConv cv = p.cv;
  int gpix[8], gih[8], giw[8], lcq[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int row = (wave * 8 + q) * 8 + lrow8;
    const int lc = w4_swz(lane & 7, row) * 8;
    const int ra = min(m0 + row, M - 1);
    lcq[q] = lc;
    oa[q] = (uint32_t)(((int64_t)ra * p.lda + lc) * 2);
    ob[q] = (uint32_t)(((int64_t)min(n0 + row, N - 1) * p.ldb + lc) * 2);
    if constexpr (SRC == 1) pa2[q] = p.A2 + xl_out_row(p.a2m, ra) * p.lda2 + lc - p.K1;
    if constexpr (SRC == 2) {
      const int hw = cv.ho * cv.wo;
      const int n = ra / hw, r = ra - n * hw, oh = r / cv.wo, ow = r - oh * cv.wo;
      gih[q] = oh * cv.stride - cv.pad;
      giw[q] = ow * cv.stride - cv.pad;
      gpix[q] = (n * cv.hi + gih[q]) * cv.wi + giw[q];
    }
  }
  const int lcz = w4_swz(lane & 7, lrow8) * 8;  // zero-row chunk (any in-bounds 16 B)
  // B rows past a narrow tile (TBN < 256) are not copied: this wave's 64 B
  // rows are either all inside or all past it
  const bool cpb = wave * 64 < TBN;
  auto dma = [&](int kt, int buf, int c) {
    const int q = c & 7;
    char* dst = smem + buf * BUF + (c >> 3) * OPB + (wave * 8 + q) * 1024;
    const int koff = kt * XBK;
    if (c >= 8 && !cpb) return;
    if (c >= 8) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsb, (lptr_t)dst, 16, ob[q], koff * 2, 0, 0);
    } else if constexpr (SRC == 2) {  // tap (tr, tc), channels c0.. of this piece's pixels, or zeros
      const int cpt = cv.cin >> 6, tap = kt / cpt, c0 = (kt - tap * cpt) << 6;
      const int tr = tap / cv.kw, tcol = tap - tr * cv.kw;
      const int ih = gih[q] + tr, iw = giw[q] + tcol;
      const bool ok = (unsigned)ih < (unsigned)cv.hi && (unsigned)iw < (unsigned)cv.wi;
      glds16(ok ? p.A + (int64_t)(gpix[q] + tr * cv.wi + tcol) * p.lda + c0 + lcq[q] : g_zero_row + lcz, dst);
    } else if constexpr (SRC == 1) {
      if (koff >= p.K1) glds16(pa2[q] + koff, dst);
      else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lptr_t)dst, 16, oa[q], koff * 2, 0, 0);
    } else {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lptr_t)dst, 16, oa[q], koff * 2, 0, 0);
    }
  };

  const int lrow = lane & 15, lk = lane >> 4;
  const int fo0 = lrow * 128 + (w4_swz(lk, lrow) << 4), fo1 = lrow * 128 + (w4_swz(4 + lk, lrow) << 4);
  const int aoff = wr * (16 * MB) * 128, boff = OPB + wc * 128 * 128;
  bf16x8 ra[2][MB], rb[2][NBW];
  // fragment read r (0..NRD-1) in the order the MFMAs consume them: A block 0,
  // B blocks 0..NBW-1, A blocks 1..MB-1
  auto rd = [&](auto hc, int buf, int r) {
    constexpr int H = decltype(hc)::value;
    const bool isb = r >= 1 && r <= NBW;
    const int blk = r == 0 ? 0 : (isb ? r - 1 : r - NBW);
    const char* base = smem + buf * BUF + (isb ? boff : aoff) + blk * 2048 + (H ? fo1 : fo0);
    if (isb) rb[H][blk] = *reinterpret_cast<const bf16x8*>(base);
    else ra[H][blk] = *reinterpret_cast<const bf16x8*>(base);
  };
  f32x4 acc[MB][NBW];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < NBW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  // operands swapped: acc[i][j] holds the transposed 16 x 16 block (lane =
  // output row i*16 + (l & 15), registers = 4 consecutive output columns),
  // the layout xl_epilogue stages as 8-B row pieces
  auto iter = [&](auto st, auto rdn, int kt) {
    constexpr bool STAGE = decltype(st)::value, READ = decltype(rdn)::value;
    const int buf = kt & 1;
    // fragment read r after MFMA (r NMF) / NRD, copy c after MFMA (c NMF) / 16:
    // spread evenly (MB = 8: a read / copy per 4 MFMAs)
#pragma unroll
    for (int n = 0; n < NMF; ++n) {
      w4_mfma(acc[n / NBW][n % NBW], rb[0][n % NBW], ra[0][n / NBW]);
      // (closed form, no inner loop: every index must fold to a constant)
      const int r = (n * NRD + NMF - 1) / NMF;  // the read r with r NMF / NRD == n, if any
      if (r < NRD && r * NMF / NRD == n) rd(I1{}, buf, r);
    }
    asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    barrier();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < NMF; ++n) {
      w4_mfma(acc[n / NBW][n % NBW], rb[1][n % NBW], ra[1][n / NBW]);
      if constexpr (STAGE) {
        const int c = (n * 16 + NMF - 1) / NMF;  // the copy c with c NMF / 16 == n, if any
        if (c < 16 && c * NMF / 16 == n) dma(kt + 2, buf, c);
      }
      if constexpr (READ)
        if ((n & 1) == 1 && (n >> 1) < NRD) rd(I0{}, buf ^ 1, n >> 1);
    }
  };
#pragma unroll
  for (int c = 0; c < 16; ++c) dma(0, 0, c);
  if (ktiles > 1) {
#pragma unroll
    for (int c = 0; c < 16; ++c) dma(1, 1, c);
    // tile 0 landed: one tile of this wave's copies (16, or 8 past a narrow B) in flight
    if (cpb) vmcnt<16>();
    else vmcnt<8>();
  } else {
    vmcnt<0>();
  }
  barrier();
  xl_mark(p, 1);
#pragma unroll
  for (int r = 0; r < NRD; ++r) rd(I0{}, 0, r);
  int kt = 0;
  for (; kt + 2 < ktiles; ++kt) iter(std::true_type{}, std::true_type{}, kt);
  if (kt + 1 < ktiles) iter(std::false_type{}, std::true_type{}, kt++);
  iter(std::false_type{}, std::false_type{}, kt);
  w4_drain();
  barrier();  // every wave is done with the operand buffers (the epilogue reuses the LDS)
  xl_mark(p, 2);
  // every copy has landed (the waits above are inline asm the compiler cannot
  // see): say so with a wait it does see (finding 66)
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  xl_epilogue<TBN, EPI, 11, LDS, MB, WN>(p, acc, smem, m0, n0, mt, mtiles, TBM);
  if (p.tdbg) {
    __syncthreads();
    xl_mark(p, 3);
  }
}

// the 4-wave kernel with the SRC its operands need: 2 = conv tap gather,
// 1 = second A source, 0 = plain
template <int EPI, int MB, int WN>
void launch_w4(const XlArgs& w, int blocks, hipStream_t s) {
  if (w.cv.cin > 0)
    hipLaunchKernelGGL((gemm_xl_w4_kernel<EPI, 2, MB, WN>), dim3(blocks), dim3(256), 0, s, w);
  else if (w.A2)
    hipLaunchKernelGGL((gemm_xl_w4_kernel<EPI, 1, MB, WN>), dim3(blocks), dim3(256), 0, s, w);
  else
    hipLaunchKernelGGL((gemm_xl_w4_kernel<EPI, 0, MB, WN>), dim3(blocks), dim3(256), 0, s, w);
}

// tile shape: a.bm came from pick_bm (the moments partials are sized by it), 224 or 256
template <int EPI>
void launch_w4_shape(const XlArgs& a, hipStream_t s) {
  const int bm = a.bm == 224 ? 224 : 256;
  const int blocks = ((a.M + bm - 1) / bm) * ((a.N + 255) / 256);
  if (a.N <= 128 && bm == 256)  // 256 x 128 tiles, the four waves along M
    launch_w4<EPI, 4, 1>(a, (a.M + 255) / 256, s);
  else if (bm == 224)
    launch_w4<EPI, 7, 2>(a, blocks, s);
  else
    launch_w4<EPI, 8, 2>(a, blocks, s);
}

}  // namespace

// (XL_AFFINE and the BN-backward epilogues are not built: w4_epi in xl_nt.h.
// XL_BNBWD with its runtime operand flags needs more registers than the
// 4-wave epilogue has: the compiler spills accumulators right behind the
// inline-asm MFMAs that write them -- read before the MFMA completes.
// tests/test_kernel_resources.py holds every gemm_xl_w4_kernel instantiation
// to zero scratch.)
void xl::launch_xl_w4(const XlArgs& a, int epi, hipStream_t s) {
  switch (epi) {
    case XL_STORE: launch_w4_shape<XL_STORE>(a, s); break;
    case XL_BIAS: launch_w4_shape<XL_BIAS>(a, s); break;
    case XL_BIAS_GELU: launch_w4_shape<XL_BIAS_GELU>(a, s); break;
    case XL_DGELU: launch_w4_shape<XL_DGELU>(a, s); break;
    case XL_BIAS_RES: launch_w4_shape<XL_BIAS_RES>(a, s); break;
    case XL_BIAS_RES_SCALE: launch_w4_shape<XL_BIAS_RES_SCALE>(a, s); break;
    case XL_MOMENTS: launch_w4_shape<XL_MOMENTS>(a, s); break;
    case XL_ADD: launch_w4_shape<XL_ADD>(a, s); break;
    default: TORCH_CHECK(false, "gemm_xl_w4_kernel: not built for epilogue ", epi);
  }
}

}  // namespace dmp
