// gemm_xl_nt_kernel: the 8-wave large-tile NT GEMM.  PIPE 10 = 256 x 256
// ping-pong quadrants (the operand-heavy conv epilogues; every 256-wide tile
// under DMP_XL_PIPE=10), PIPE 1 / 0 = the ring and two-buffer loops (256 x 128
// tiles and A/B options).  Epilogues, arguments and xl_epilogue: xl_nt.h; the
// host side that routes launches here: gemm_xl.hip.
//
// Structure (cdna_hip_programming.md §5 "256² template" and T1-T5):
//   * 256 x BN tile (BN = 256 or 128), BK = 64, 512 threads = 8 waves as
//     2 (M) x 4 (N); each wave owns 128 x BN/4 outputs = 8 x BN/64 16x16
//     accumulators (v_mfma_f32_16x16x32_bf16);
//   * operands staged global -> LDS by global_load_lds_dwordx4 (no VGPR
//     round trip); the LDS image is lane-linear, so the bank swizzle is applied
//     to the per-lane SOURCE address and undone on the ds_read (rule 21);
//   * every K tile is split into two k32 halves living in their own LDS
//     regions ([A|B] x [k0|k1] x 2 buffers = 128 KB at BN = 256); one K tile is
//     4 phases (k-half x M-half of the wave tile, 16 / 8 MFMAs each), and each
//     phase issues the global->LDS copy of one region as soon as that region's
//     previous contents were consumed: the k0 halves of tile t+2 are issued
//     while tile t computes its k1 half, so ~5 phases of loads stay in flight
//     across the barriers (counted s_waitcnt vmcnt, raw s_barrier -- never
//     __syncthreads, whose fence would drain the DMA queue);
//   * one raw s_barrier per phase; the region written in phase p was last read
//     before the previous phase's barrier (WAR), and a region is read one phase
//     after the vmcnt that retired it (RAW);
//   * bijective XCD-aware block remap (T1); the N tiles of an M tile are
//     adjacent (they share the A panel in L2);
//   * epilogue restages the tile through LDS for 16-B row-contiguous stores.
#include <type_traits>
#include "xl_nt.h"

namespace dmp {
namespace {

template <int BN, int EPI, int PIPE>
__global__ __launch_bounds__(XTHREADS, 1) void gemm_xl_nt_kernel(const XlArgs p) {
  constexpr int WTM = 128, WTN = BN / 4;
  constexpr int MI = WTM / 16, NI = WTN / 16;       // 8 x (4 | 2) accumulators
  constexpr int RA = XBM * 64, RB = BN * 64;        // bytes of one k32 region
  constexpr int NA = RA / 1024 / 8, NB = RB / 1024 / 8;  // glds per wave per region
  constexpr int STAGE_LDS = 4 * RA + 4 * RB;
  constexpr int CT_STRIDE = BN + 8;
  constexpr int EPI_LDS = XBM * CT_STRIDE * 2;
  constexpr int LDS = STAGE_LDS > EPI_LDS ? STAGE_LDS : EPI_LDS;
  constexpr int W2 = 2 * (NA + NB);  // glds per wave per K tile
  static_assert(NA >= 1 && NB >= 1, "region smaller than one glds round");
  __shared__ __attribute__((aligned(16))) char smem[LDS];
  // XL_DGELU: column sums of the output (fc1's bias gradient) when p.part is set
  constexpr bool kMom = EPI == XL_MOMENTS || is_bnbwd(EPI) || EPI == XL_DGELU;
  if constexpr (kMom) zero_moments(p.zsums, 2 * p.N);

  const bf16* __restrict__ A = p.A;
  const bf16* __restrict__ B = p.B;
  const int64_t lda = p.lda, ldb = p.ldb;
  const int M = p.M, N = p.N, K = p.K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int tbm = (PIPE == 10 && p.bm > 0) ? p.bm : XBM;  // rows per tile (pick_bm)
  const int mtiles = (M + tbm - 1) / tbm, ntiles = (N + BN - 1) / BN;
  int mt, nt;
  tile_coords(mtiles * ntiles, mtiles, ntiles, p.group_m, mt, nt);
  const int m0 = mt * tbm, n0 = nt * BN;
  const int ktiles = K / XBK;
  if (p.tdbg && threadIdx.x == 0) {
    p.tdbg[(int64_t)blockIdx.x * 8 + 0] = __builtin_amdgcn_s_memrealtime();
    p.tdbg[(int64_t)blockIdx.x * 8 + 4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
    p.tdbg[(int64_t)blockIdx.x * 8 + 5] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
  }

  // ---- staging: lane L of a 1 KB glds instruction writes LDS bytes L*16..+16
  // of 16 rows x 64 B; the logical 16-B chunk it carries is the physical one
  // XOR swz(row) (row & 15 = L >> 2, so the XOR depends on L >> 4 only).
  const int srow = lane >> 2;
  const int schunk = (lane & 3) ^ chunk_xor(lane >> 4);
  const bf16* asrc[NA];
  const bf16* asrc2[NA];
  const bf16* bsrc[NB];
#pragma unroll
  for (int q = 0; q < NA; ++q) {
    const int r = (wave * NA + q) * 16 + srow;
    asrc[q] = A + (int64_t)min(m0 + r, M - 1) * lda + schunk * 8;
    asrc2[q] = p.A2 ? p.A2 + xl_out_row(p.a2m, min(m0 + r, M - 1)) * p.lda2 + schunk * 8 - p.K1 : nullptr;
  }
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int r = (wave * NB + q) * 16 + srow;
    bsrc[q] = B + (int64_t)min(n0 + r, N - 1) * ldb + schunk * 8;
  }
  auto a_region = [&](int ks, int buf) { return smem + (buf * 2 + ks) * RA; };
  auto b_region = [&](int ks, int buf) { return smem + 4 * RA + (buf * 2 + ks) * RB; };
  auto stage_a = [&](int ks, int kt, int buf) {
    char* dst = a_region(ks, buf) + wave * NA * 1024;
    const int koff = kt * XBK + ks * 32;
    const bool second = p.A2 && koff >= p.K1;
#pragma unroll
    for (int q = 0; q < NA; ++q) glds16((second ? asrc2[q] : asrc[q]) + koff, dst + q * 1024);
  };
  auto stage_b = [&](int ks, int kt, int buf) {
    char* dst = b_region(ks, buf) + wave * NB * 1024;
    const int koff = kt * XBK + ks * 32;
#pragma unroll
    for (int q = 0; q < NB; ++q) glds16(bsrc[q] + koff, dst + q * 1024);
  };

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lrow = lane & 15, lk = lane >> 4;
  // fragment byte offset of row r (multiple of 16 + lrow) in a k32 region
  const int frag_off = lrow * 64 + ((lk ^ chunk_xor(lrow >> 2)) << 4);
  bf16x8 fb[NI];

  auto phase = [&](int ks, int mh, int buf) {
    const char* ar = a_region(ks, buf) + (wr * WTM + mh * 64) * 64 + frag_off;
    bf16x8 fa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(ar + i * 16 * 64);
    if (mh == 0) {
      const char* br = b_region(ks, buf) + (wc * WTN) * 64 + frag_off;
#pragma unroll
      for (int j = 0; j < NI; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(br + j * 16 * 64);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
        acc[mh * 4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[mh * 4 + i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  if constexpr (PIPE == 0) {
  // ---- prologue: tile 0 (both halves) and tile 1's k0 half in flight ----
  stage_a(0, 0, 0);
  stage_b(0, 0, 0);
  stage_a(1, 0, 0);
  stage_b(1, 0, 0);
  if (ktiles > 1) {
    stage_a(0, 1, 1);
    stage_b(0, 1, 1);
    vmcnt<W2>();
  } else {
    vmcnt<NA + NB>();
  }
  barrier();

  for (int kt = 0; kt < ktiles; ++kt) {
    const int buf = kt & 1;
    const bool has1 = kt + 1 < ktiles, has2 = kt + 2 < ktiles;
    // phase 0: k0 half, M half 0; stage tile kt+1's A k1 half
    if (has1) stage_a(1, kt + 1, buf ^ 1);
    phase(0, 0, buf);
    barrier();
    // phase 1: k0, M half 1; stage tile kt+1's B k1; retire tile kt's k1 half
    if (has1) stage_b(1, kt + 1, buf ^ 1);
    phase(0, 1, buf);
    if (has1) vmcnt<W2>(); else vmcnt<0>();
    barrier();
    // phase 2: k1, M half 0; this tile's k0 regions are free: stage tile kt+2's A k0
    if (has2) stage_a(0, kt + 2, buf);
    phase(1, 0, buf);
    barrier();
    // phase 3: k1, M half 1; stage kt+2's B k0; retire tile kt+1's k0 half
    if (has2) stage_b(0, kt + 2, buf);
    phase(1, 1, buf);
    if (has2) vmcnt<W2>(); else if (has1) vmcnt<NA + NB>(); else vmcnt<0>();
    barrier();
  }
  } else if constexpr (PIPE == 10) {
  // ---- PIPE 10: ping-pong quadrant schedule (cdna_hip_programming.md §5 "256²
  // 8-phase template").  The two wave rows (wr) run one barrier apart: while
  // one group's 4 waves run a phase's 16 MFMAs, the other group (one wave on
  // each SIMD) issues that phase's ds_reads and LDS-DMA copies, so every SIMD
  // alternates a MFMA wave and a memory wave between consecutive barriers.
  // A K tile is 4 phases, one per quadrant (m half, n half) of the wave's
  // 128 x 64 outputs, in the order (0,0) (0,1) (1,1) (1,0) so that each phase
  // re-reads only one operand.  A tile's operands are staged as 4 units of
  // 16 KB (2 glds per wave): U0 = A rows of m half 0, U3 = m half 1, U1 = B
  // cols of n half 0, U2 = n half 1.  Which phase stages and retires which
  // unit is in the unit schedule before the main loop below (RAW: the counted
  // wait -- never 0 in steady state -- then a barrier, then the ds_read).
  static_assert(BN == 256, "ping-pong schedule is written for 256 x 256 tiles");
  const int pks = wave >> 2;  // k32 half carried by this wave's two copies of a unit
  const bf16* pa[2][2];
  const bf16* pa2[2][2];
  const bf16* pb[2][2];
  int oa[2][2], ob[2][2];
#pragma unroll
  for (int v = 0; v < 2; ++v)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int j = (2 * wave + q) & 7;
      const int ba = (j & 3) + 8 * (j >> 2) + 4 * v, bb = (j & 1) + 4 * (j >> 1) + 2 * v;
      pa[v][q] = A + (int64_t)min(m0 + ba * 16 + srow, M - 1) * lda + schunk * 8 + pks * 32;
      pa2[v][q] = p.A2 ? p.A2 + xl_out_row(p.a2m, min(m0 + ba * 16 + srow, M - 1)) * p.lda2 + schunk * 8 + pks * 32 -
                             p.K1
                       : nullptr;
      pb[v][q] = B + (int64_t)min(n0 + bb * 16 + srow, N - 1) * ldb + schunk * 8 + pks * 32;
      oa[v][q] = ba * 1024;
      ob[v][q] = bb * 1024;
    }
  // conv gather: per staged A row, its top-left input pixel and coordinates
  const XlConv cv = p.cv;
  const bool gather = cv.cin > 0;
  const int loff = schunk * 8 + pks * 32;
  int gpix[2][2], gih[2][2], giw[2][2];
  if (gather) {
    const int hw = cv.ho * cv.wo;
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int j = (2 * wave + q) & 7;
        const int row = min(m0 + ((j & 3) + 8 * (j >> 2) + 4 * v) * 16 + srow, M - 1);
        const int n = row / hw, r = row - n * hw, oh = r / cv.wo, ow = r - oh * cv.wo;
        gih[v][q] = oh * cv.stride - cv.pad;
        giw[v][q] = ow * cv.stride - cv.pad;
        gpix[v][q] = (n * cv.hi + gih[v][q]) * cv.wi + giw[v][q];
      }
  }
  auto stage_unit = [&](auto u, int kt) {
    constexpr int U = decltype(u)::value;
    const int buf = kt & 1, koff = kt * XBK;
    if constexpr (U == 0 || U == 3) {
      if (gather) {  // tap (tr, tc), channels c0.. of every staged output pixel, or zeros
        const int cpt = cv.cin >> 6, tap = kt / cpt, c0 = (kt - tap * cpt) << 6;
        const int tr = tap / cv.kw, tc = tap - tr * cv.kw;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int ih = gih[U == 3][q] + tr, iw = giw[U == 3][q] + tc;
          const bool ok = (unsigned)ih < (unsigned)cv.hi && (unsigned)iw < (unsigned)cv.wi;
          const bf16* src = ok ? A + (int64_t)(gpix[U == 3][q] + tr * cv.wi + tc) * lda + c0 + loff
                               : g_zero_row + loff;
          glds16(src, a_region(pks, buf) + oa[U == 3][q]);
        }
        return;
      }
    }
    const bool second = p.A2 && koff >= p.K1;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if constexpr (U == 0 || U == 3)
        glds16((second ? pa2[U == 3][q] : pa[U == 3][q]) + koff, a_region(pks, buf) + oa[U == 3][q]);
      else
        glds16(pb[U == 2][q] + koff, b_region(pks, buf) + ob[U == 2][q]);
    }
  };
  // PIPE 10 keeps both n halves of B in registers (qb[nq]): B half 0 is
  // read once per K tile instead of twice, so every unit has one reader phase
  // and its slot frees two phases earlier -- the copies are issued 4 phases
  // ahead of their readers instead of 2 (vmcnt(8): 64 KB in flight per wave
  // group instead of 32 KB; the round-4 schedule that re-read B's n half 0
  // was PIPE 7, removed)
  bf16x8 qa[2][4], qb[2][2][2];
  auto read_a = [&](int mq, int buf) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        qa[ks][i] = *reinterpret_cast<const bf16x8*>(a_region(ks, buf) + (wr * WTM + mq * 64 + i * 16) * 64 + frag_off);
  };
  auto read_b = [&](int nq, int buf) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        qb[nq][ks][j] =
            *reinterpret_cast<const bf16x8*>(b_region(ks, buf) + (wc * WTN + nq * 32 + j * 16) * 64 + frag_off);
  };
  // a trimmed tile (tbm < 256, >= 192): wave row 1's m-half-1 blocks past
  // row tbm are the next tile's rows -- their MFMAs are skipped (wave-uniform)
  const int ilim = wr ? ((tbm - 192) >> 4) : 4;
  auto quad = [&](auto mqc, auto nqc) {
    constexpr int MQ = decltype(mqc)::value, NQ = decltype(nqc)::value;
    barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    // operands swapped: acc holds C^T blocks (lane = output row, registers =
    // 4 consecutive output columns), so the epilogue stages 8-B row pieces
    if (MQ == 0 || ilim >= 4) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[MQ * 4 + i][NQ * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                qb[NQ][ks][j], qa[ks][i], acc[MQ * 4 + i][NQ * 2 + j], 0, 0, 0);
    } else {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < ilim) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
              acc[MQ * 4 + i][NQ * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  qb[NQ][ks][j], qa[ks][i], acc[MQ * 4 + i][NQ * 2 + j], 0, 0, 0);
          }
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    barrier();
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  // ---- PIPE 10 unit schedule (K tile kt lives in buffer kt & 1).  Readers: U0, U1 of tile t in phase 0 (quad
  // (0,0)), U2 in phase 1, U3 in phase 2; phase 3 reads nothing.  Phase r of
  // tile t stages U2(t+1), U3(t+1), U0(t+2), U1(t+2): each is written >= 2
  // phases after its slot's previous reader (WAR) and retired by a vmcnt 4
  // phases after its issue, one phase before its reader (RAW).  The waits
  // leave the 4 youngest units (8 copies per wave) in flight; phase 2 has no
  // reader in the next phase and so no wait.
  stage_unit(I0{}, 0);
  stage_unit(I1{}, 0);
  stage_unit(I2{}, 0);
  stage_unit(I3{}, 0);
  if (ktiles > 1) {
    stage_unit(I0{}, 1);
    stage_unit(I1{}, 1);
    vmcnt<8>();
  } else {
    vmcnt<4>();
  }
  barrier();
  xl_mark(p, 1);
  if (wr == 1) barrier();  // the stagger: wave row 1 runs one barrier behind
  for (int kt = 0; kt < ktiles; ++kt) {
    const int buf = kt & 1;
    const bool n1 = kt + 1 < ktiles, n2 = kt + 2 < ktiles;
    read_a(0, buf);
    read_b(0, buf);
    if (n1) { stage_unit(I2{}, kt + 1); vmcnt<8>(); } else { vmcnt<2>(); }
    quad(I0{}, I0{});
    read_b(1, buf);
    if (n1) { stage_unit(I3{}, kt + 1); vmcnt<8>(); } else { vmcnt<0>(); }
    quad(I0{}, I1{});
    read_a(1, buf);
    if (n2) stage_unit(I0{}, kt + 2);
    quad(I1{}, I1{});
    if (n2) { stage_unit(I1{}, kt + 2); vmcnt<8>(); } else if (n1) { vmcnt<4>(); } else { vmcnt<0>(); }
    quad(I1{}, I0{});
  }
  if (wr == 0) barrier();  // equal barrier counts before the epilogue
  barrier();
  xl_mark(p, 2);
  } else {
  // ---- PIPE 1: half-step ring.  Half-step s (K tile s/2, k32 half s%2) lives
  // in LDS region s%4.  During half-step s: stage region s%4 with the data of
  // half-step s+4 (its fragments were read in s-1 and retired before that
  // step's barrier), ds_read the fragments of s+1 into the other register set
  // (retired by the vmcnt at the end of s-1), run the 32 MFMAs of s.  One
  // barrier per half-step; three half-steps of copies in flight.
  const int S = 2 * ktiles;
  auto stage_h = [&](int h) {
    stage_a(h & 1, h >> 1, (h >> 1) & 1);
    stage_b(h & 1, h >> 1, (h >> 1) & 1);
  };
  bf16x8 xa[MI], xb[NI], ya[MI], yb[NI];
  auto read_frags = [&](bf16x8 (&fa)[MI], bf16x8 (&fbb)[NI], int h) {
    const char* ar = smem + (h & 3) * RA + (wr * WTM) * 64 + frag_off;
    const char* br = smem + 4 * RA + (h & 3) * RB + (wc * WTN) * 64 + frag_off;
#pragma unroll
    for (int j = 0; j < NI; ++j) fbb[j] = *reinterpret_cast<const bf16x8*>(br + j * 16 * 64);
#pragma unroll
    for (int i = 0; i < MI; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(ar + i * 16 * 64);
  };
  auto mfmas = [&](const bf16x8 (&fa)[MI], const bf16x8 (&fbb)[NI]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fbb[j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  auto lgkm0 = [] { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
  // prologue: half-steps 0..3 in flight; retire 0, read it, retire 1
  stage_h(0);
  stage_h(1);
  if (S >= 4) {
    stage_h(2);
    stage_h(3);
    vmcnt<3 * (NA + NB)>();
  } else {
    vmcnt<NA + NB>();
  }
  barrier();
  read_frags(xa, xb, 0);
  if (S >= 4) vmcnt<2 * (NA + NB)>(); else vmcnt<0>();
  lgkm0();
  barrier();
  for (int s = 0; s < S; s += 2) {
    if (s + 4 < S) stage_h(s + 4);
    read_frags(ya, yb, s + 1);
    mfmas(xa, xb);
    if (s + 4 < S) vmcnt<2 * (NA + NB)>(); else vmcnt<0>();
    lgkm0();
    barrier();
    if (s + 5 < S) stage_h(s + 5);
    if (s + 2 < S) read_frags(xa, xb, s + 2);
    mfmas(ya, yb);
    if (s + 5 < S) vmcnt<2 * (NA + NB)>(); else vmcnt<0>();
    lgkm0();
    barrier();
  }
  }

  // ---- epilogue: (acc [+ bias]) -> bf16 tile in LDS, then row-contiguous pass ----
  // every operand copy has landed (the main loops end on vmcnt(0) in inline
  // asm, which the compiler cannot see): say so with a wait it does see, or it
  // drains the epilogue's first operand batch before its first LDS write to
  // order that write after the copies into LDS
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  xl_epilogue<BN, EPI, PIPE, LDS>(p, acc, smem, m0, n0, mt, mtiles, tbm);
  if (p.tdbg) {
    __syncthreads();
    xl_mark(p, 3);
  }
}

// The PIPEs built per epilogue: 10 at 256-wide tiles only; the conv epilogues
// (!is_linear_epi) have no two-buffer (PIPE 0) form.
template <int EPI>
void launch_nt8(const XlArgs& a, int bn, int pipe, int blocks, hipStream_t s) {
  const dim3 grid(blocks), block(XTHREADS);
  constexpr bool kTwoBuf = is_linear_epi(EPI);
  TORCH_CHECK((bn == 128 || bn == 256) && (pipe == 1 || (pipe == 10 && bn == 256) || (pipe == 0 && kTwoBuf)),
              "gemm_xl_nt_kernel: not built for epilogue ", EPI, " at bn ", bn, ", pipe ", pipe);
  if (pipe == 10) {
    hipLaunchKernelGGL((gemm_xl_nt_kernel<256, EPI, 10>), grid, block, 0, s, a);
  } else if (pipe == 1) {
    if (bn == 256) hipLaunchKernelGGL((gemm_xl_nt_kernel<256, EPI, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((gemm_xl_nt_kernel<128, EPI, 1>), grid, block, 0, s, a);
  } else if constexpr (kTwoBuf) {
    if (bn == 256) hipLaunchKernelGGL((gemm_xl_nt_kernel<256, EPI, 0>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((gemm_xl_nt_kernel<128, EPI, 0>), grid, block, 0, s, a);
  }
}

}  // namespace

void xl::launch_xl_nt8(const XlArgs& a, int epi, int bn, int pipe, int blocks, hipStream_t s) {
  switch (epi) {
    case XL_STORE: launch_nt8<XL_STORE>(a, bn, pipe, blocks, s); break;
    case XL_BIAS: launch_nt8<XL_BIAS>(a, bn, pipe, blocks, s); break;
    case XL_BIAS_GELU: launch_nt8<XL_BIAS_GELU>(a, bn, pipe, blocks, s); break;
    case XL_DGELU: launch_nt8<XL_DGELU>(a, bn, pipe, blocks, s); break;
    case XL_BIAS_RES: launch_nt8<XL_BIAS_RES>(a, bn, pipe, blocks, s); break;
    case XL_BIAS_RES_SCALE: launch_nt8<XL_BIAS_RES_SCALE>(a, bn, pipe, blocks, s); break;
    case XL_MOMENTS: launch_nt8<XL_MOMENTS>(a, bn, pipe, blocks, s); break;
    case XL_ADD: launch_nt8<XL_ADD>(a, bn, pipe, blocks, s); break;
    case XL_BNBWD: launch_nt8<XL_BNBWD>(a, bn, pipe, blocks, s); break;
    case XL_AFFINE: launch_nt8<XL_AFFINE>(a, bn, pipe, blocks, s); break;
    case XL_BNBWD_Y: launch_nt8<XL_BNBWD_Y>(a, bn, pipe, blocks, s); break;
    case XL_BNBWD_YO: launch_nt8<XL_BNBWD_YO>(a, bn, pipe, blocks, s); break;
    default: TORCH_CHECK(false, "gemm_xl_nt_kernel: unknown epilogue ", epi);
  }
}

}  // namespace dmp
