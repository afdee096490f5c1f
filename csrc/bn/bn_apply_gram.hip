// Training-mode BN apply + ReLU that also forms the Gram matrix of its output.
//
// The bottleneck whose bn3 is folded through conv3 (ops/bn_fold.py) needs, of
// a2 = relu(bn2(y2)) [M, C], the column sums and G = a2^T a2.  The apply pass
// (batchnorm.hip bn_apply_kernel, OSUM) already reduced the column sums; G
// was a second full read of a2 by the TN GEMM.  Here every block forms its
// slab's share of G from the values it has just normalised:
//   * a block of 4 waves owns a contiguous slab of rows and walks it in steps
//     of 64 rows.  Per step every lane loads its C / 32 16-B vectors (lane ->
//     one 8-channel vector of a row, as in bn_apply_kernel, so the per-channel
//     coefficients stay in registers), transforms them, stores them to `a`
//     and writes the same bf16 values into an LDS tile [64 rows][C];
//   * the tile is C / 64 planes of [64 rows][64 cols] (128-B rows), 16-B chunk
//     c of row r at c ^ swz(r): the image gemm_tn_w4_kernel reads its
//     ds_read_b64_tr_b16 fragments from without bank conflicts, and one that
//     8 consecutive lanes' ds_write_b128 (one row's 128 B) fill without any;
//   * the C x C accumulator is split 2 x 2 over the waves (C / 32 x C / 32
//     16 x 16 blocks each: 16 / 64 / 256 registers at C = 64 / 128 / 256, the
//     last in AGPRs through w4_mfma).  The A and B fragments of G are the same
//     data: a fragment is "8 consecutive rows of one column", whichever side
//     of the MFMA it feeds;
//   * the tile is double-buffered with ONE barrier per step: the loads of
//     step t + 1 are issued before step t is transformed, so they and the
//     stores of step t are in flight under step t's MFMAs;
//   * rows past the slab's end enter the tile as zeros (not relu(shift));
//   * every block writes an fp32 partial of G ([blocks][C][C]) that
//     split_reduce_launch sums, and a partial row of the column sums that
//     bn_reduce_partials_launch reduces in fp64: no float atomics, the fold's
//     statistics repeat from run to run.  The grid is sized per C so that the
//     partials stay small against the pass.
// `a`, mean, invstd and the running statistics are bit-identical to
// bn_forward_apply's: same fwd_coeffs, same fmaf, clamp and rounding.
#include <algorithm>
#include <type_traits>

#include <ATen/hip/HIPContext.h>
#include "../api.h"
#include "../launch.h"
#include "../gemm/xl_common.h"
#include "bn_coeffs.h"

namespace dmp {
namespace {

constexpr int kGThreads = 256, kGStep = 64;

// 16-B chunk swizzle of a 128-B plane row (gemm_tn_xl.hip tnw_swz)
__device__ __forceinline__ int gram_swz(int row) { return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2); }

template <int C, bool NT>
__global__ __launch_bounds__(kGThreads, 256 / C) void bn_apply_gram_kernel(
    const bf16* __restrict__ x, const double* __restrict__ sums, const float* __restrict__ weight,
    const float* __restrict__ bias, float* __restrict__ running_mean, float* __restrict__ running_var,
    float momentum, float eps, int64_t M, int64_t rows_per_block, bf16* __restrict__ y,
    float* __restrict__ save_mean, float* __restrict__ save_invstd, int64_t* __restrict__ num_batches_tracked,
    float* __restrict__ opart, double* __restrict__ ozsums, float* __restrict__ gpart, float clip) {
  constexpr int TC = C / 8;               // lanes (16-B vectors) per row
  constexpr int RPI = kGThreads / TC;     // rows per block-wide load
  constexpr int L = kGStep / RPI;         // loads per lane and step
  constexpr int PLANE = 64 * 128;         // bytes: [64 rows][64 cols]
  constexpr int BUF = (C / 64) * PLANE;   // one tile
  constexpr int MB = C / 32;              // 16 x 16 blocks per wave and side
  static_assert(2 * BUF >= 2 * 8 * kGThreads * 4, "the column-sum combine reuses the tiles");
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  using v4i16 = short __attribute__((ext_vector_type(4)));
  using lds_v4 = __attribute__((address_space(3))) v4i16;

  if (num_batches_tracked != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *num_batches_tracked += 1;
  zero_moments(ozsums, 2 * C);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int lc = tid % TC, lr = tid / TC;

  float sc[8], sh[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lc * 8 + i;
    float mean, invstd, var_b;
    fwd_coeffs(sums, C, c, weight, bias, eps, mean, invstd, var_b, sc[i], sh[i]);
    if (blockIdx.x == 0 && lr == 0) {
      save_mean[c] = mean;
      save_invstd[c] = invstd;
      if (running_mean) {
        const double n = sums[2 * C];
        const float unb = n > 1.0 ? (float)((double)var_b * n / (n - 1.0)) : var_b;
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * unb;
      }
    }
  }

  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(M, r0 + rows_per_block);
  const int nsteps = (int)((r1 - r0 + kGStep - 1) / kGStep);
  const bf16* xp = x + (r0 + lr) * C + lc * 8;
  bf16* yp = y + (r0 + lr) * C + lc * 8;
  const int64_t nrow = r1 - r0;

  // this lane's slot of tile row it * RPI + lr
  int soff[L];
#pragma unroll
  for (int it = 0; it < L; ++it) {
    const int r = it * RPI + lr;
    soff[it] = (lc >> 3) * PLANE + r * 128 + (((lc & 7) ^ gram_swz(r)) << 4);
  }
  // PRED: rows past the slab's end are not read (zeros) / not stored; the
  // steps of the main loop are whole, and their code is free of branches, so
  // the compiler's vmcnt waits stay counted (a load under a branch made it
  // wait for everything in flight, the stores included, every step)
  auto load = [&](bf16x8 (&v)[L], int t, auto pred) __attribute__((always_inline)) {
    constexpr bool PRED = decltype(pred)::value;
#pragma unroll
    for (int it = 0; it < L; ++it) {
      const int64_t r = (int64_t)t * kGStep + it * RPI + lr;  // within the slab
      bf16x8 z = {};
      if (!PRED || r < nrow) {
        const bf16x8* p = reinterpret_cast<const bf16x8*>(xp + (r - lr) * C);
        z = NT ? __builtin_nontemporal_load(p) : *p;
      }
      v[it] = z;
    }
    // the loads stay where they are written, ahead of the step they run
    // under (at C = 128 the scheduler sank them below that step's stores)
    if constexpr (!PRED) __builtin_amdgcn_sched_barrier(0);
  };

  // transposing fragment read (gemm_tn_w4_kernel's tr_frag): the 8 rows
  // 32 h + 8 g .. + 7 of column col + (lane & 15)
  const int g = lane >> 4, li = lane & 15, q4 = li >> 2, p4 = li & 3;
  auto tr_frag = [&](const char* tile, int h, int col) __attribute__((always_inline)) {
    const char* plane = tile + (col >> 6) * PLANE;
    const int rr0 = h * 32 + 8 * g + q4, rr1 = rr0 + 4;
    const int cb = ((col & 63) + 4 * p4) * 2;
    const char* a0 = plane + rr0 * 128 + ((((cb >> 4) ^ gram_swz(rr0))) << 4) + (cb & 15);
    const char* a1 = plane + rr1 * 128 + ((((cb >> 4) ^ gram_swz(rr1))) << 4) + (cb & 15);
    v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)a0);
    v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)a1);
    short __attribute__((ext_vector_type(8))) t8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, t8);
  };

  f32x4 acc[MB][MB];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < MB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (C == 256) {
    // the zeros are written HERE: left to itself the compiler wrote each
    // accumulator right in front of the first w4_mfma that reads it, and an
    // inline-asm MFMA gets no hazard wait states after such a write (one
    // 16 x 16 block of G came out as stale register contents)
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int j = 0; j < MB; ++j) asm volatile("" : "+a"(acc[i][j]));
    w4_drain();
  }
  float os[8], oq[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { os[i] = 0.f; oq[i] = 0.f; }

  // one step: transform and store the rows in `v`, fill tile t & 1, then the
  // MFMAs of the tile
  auto step = [&](bf16x8 (&v)[L], int t, auto pred) __attribute__((always_inline)) {
    constexpr bool PRED = decltype(pred)::value;
    char* tile = smem + (t & 1) * BUF;
#pragma unroll
    for (int it = 0; it < L; ++it) {
      const int64_t r = (int64_t)t * kGStep + it * RPI + lr;
      const bool ok = !PRED || r < nrow;
      const f32x8 f = __builtin_convertvector(v[it], f32x8);
      f32x8 o;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = fminf(fmaxf(fmaf(f[i], sc[i], sh[i]), 0.f), clip);
      bf16x8 ob = __builtin_convertvector(o, bf16x8);
      if (!ok) ob = bf16x8{};  // a row past the slab is zero in the tile, not relu(shift)
      const f32x8 s = __builtin_convertvector(ob, f32x8);  // the values as stored
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        os[i] += s[i];
        oq[i] = fmaf(s[i], s[i], oq[i]);
      }
      if (ok) {
        bf16x8* p = reinterpret_cast<bf16x8*>(yp + (r - lr) * C);
        if (NT) __builtin_nontemporal_store(ob, p);
        else *p = ob;
      }
      *reinterpret_cast<bf16x8*>(tile + soff[it]) = ob;
    }
    // the tile is written: one barrier per step (the other tile's readers of
    // step t - 1 are all past it before any wave writes that tile in t + 1)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    barrier();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // the A and B fragments of G are the same kind of data; a diagonal wave
      // reads its own twice (a uniform branch here cost more than the reads)
      bf16x8 fa[MB], fb[MB];
#pragma unroll
      for (int i = 0; i < MB; ++i) fa[i] = tr_frag(tile, h, (wr * MB + i) * 16);
#pragma unroll
      for (int j = 0; j < MB; ++j) fb[j] = tr_frag(tile, h, (wc * MB + j) * 16);
      // operands swapped as in gemm_tn_w4_kernel: lane = row of G (i side),
      // registers = 4 consecutive columns (j side)
#pragma unroll
      for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < MB; ++j) {
          if constexpr (C == 256) w4_mfma(acc[i][j], fb[j], fa[i]);
          else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
      // one half's fragments live at a time (both, hoisted, spilled at C = 128)
      if constexpr (C == 128) __builtin_amdgcn_sched_barrier(0);
    }
  };

  // two register sets in turn: the loads of step t + 1 are issued before step
  // t is transformed.  Whole steps two at a time without a branch inside, then
  // the (at most three) last ones with the row checks.
  const int nfull = (int)(nrow / kGStep);
  bf16x8 va[L], vb[L];
  int t = 0;
  if (nfull >= 3) {
    // the first pair outside the loop: the loop is then entered with what
    // every later pair leaves in flight (va's loads, then a step's stores),
    // and its first wait is a counted one, not vmcnt(0)
    load(va, 0, std::false_type{});
    load(vb, 1, std::false_type{});
    step(va, 0, std::false_type{});
    load(va, 2, std::false_type{});
    step(vb, 1, std::false_type{});
    for (t = 2; t + 2 < nfull; t += 2) {
      load(vb, t + 1, std::false_type{});
      step(va, t, std::false_type{});
      load(va, t + 2, std::false_type{});
      step(vb, t + 1, std::false_type{});
    }
  } else {
    load(va, 0, std::true_type{});
  }
  for (; t < nsteps; ++t) {
    if (t + 1 < nsteps) load(vb, t + 1, std::true_type{});
    step(va, t, std::true_type{});
#pragma unroll
    for (int it = 0; it < L; ++it) va[it] = vb[it];
  }
  if constexpr (C == 256) w4_drain();

  // this block's fp32 partial of G
  float* gp = gpart + (int64_t)blockIdx.x * C * C;
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    const int n = (wr * MB + i) * 16 + li;
#pragma unroll
    for (int j = 0; j < MB; ++j) {
      const int k = (wc * MB + j) * 16 + g * 4;
      *reinterpret_cast<f32x4*>(gp + n * C + k) = acc[i][j];
    }
  }

  // column sums: combine the RPI row-lanes of each channel through the
  // (now free) tiles, one partial row per block (batchnorm.hip block_combine_store)
  barrier();
  float* lds_s = reinterpret_cast<float*>(smem);
  float* lds_q = lds_s + 8 * kGThreads;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    lds_s[i * kGThreads + tid] = os[i];
    lds_q[i * kGThreads + tid] = oq[i];
  }
  __syncthreads();
  for (int o = tid; o < C; o += kGThreads) {
    const int c_l = o % TC, e = o / TC;
    float ss = 0.f, qq = 0.f;
    for (int rr = 0; rr < RPI; ++rr) {
      ss += lds_s[e * kGThreads + rr * TC + c_l];
      qq += lds_q[e * kGThreads + rr * TC + c_l];
    }
    opart[(int64_t)blockIdx.x * C + c_l * 8 + e] = ss;
    opart[(int64_t)(gridDim.x + blockIdx.x) * C + c_l * 8 + e] = qq;
  }
}

int g_gram_blocks = 0;  // 0: per-C default; else the target grid (set_bn_gram_blocks, sweeps)

// Blocks per C: the fp32 partials of G cost blocks * C^2 * 4 B written and
// read again -- 8 / 16 / 64 MB at the defaults, against a pass of 1644 / 822 /
// 411 MB over a ResNet-50 layer-1 / 2 / 3 activation at batch 2048.  Measured
// there (tools/bn_gram_bench.py, profiles/bn_apply_gram.md): 256 / 512 / 1024 /
// 2048 blocks take 0.340 / 0.338 / 0.346 / 0.344 ms at C = 64, 0.178 / 0.183 /
// 0.184 / 0.192 ms at C = 128 and 0.116 / 0.141 / 0.200 / 0.282 ms at C = 256.
int gram_target_blocks(int C) {
  if (g_gram_blocks > 0) return g_gram_blocks;
  return C == 64 ? 512 : 256;
}

float* gfptr(const c10::optional<at::Tensor>& t) {
  return (t.has_value() && t->defined()) ? t->data_ptr<float>() : nullptr;
}

}  // namespace

bool bn_apply_gram_supported(int64_t C) { return C == 64 || C == 128 || C == 256; }
void set_bn_gram_blocks(int64_t n) { g_gram_blocks = (int)n; }

// bn_forward_apply(..., relu, out_moments) that also returns G = a^T a (fp32
// [C, C]) of the stored output: {a, mean, invstd, osums, G}.
std::vector<at::Tensor> bn_forward_apply_gram(const at::Tensor& x, const at::Tensor& sums,
                                              const c10::optional<at::Tensor>& weight,
                                              const c10::optional<at::Tensor>& bias,
                                              const c10::optional<at::Tensor>& running_mean,
                                              const c10::optional<at::Tensor>& running_var, double momentum,
                                              double eps, int64_t C,
                                              const c10::optional<at::Tensor>& num_batches_tracked, double clip) {
  TORCH_CHECK(bn_apply_gram_supported(C), "bn_forward_apply_gram: C must be 64, 128 or 256");
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous() && x.numel() % C == 0,
              "bn_forward_apply_gram: x must be a contiguous bf16 [M, C] GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "bn_forward_apply_gram: x must be 16-B aligned");
  TORCH_CHECK(sums.is_cuda() && sums.scalar_type() == at::kDouble && sums.numel() == 2 * C + 1 &&
                  sums.is_contiguous(), "bad moments");
  auto check_c = [&](const c10::optional<at::Tensor>& t, const char* name) {
    TORCH_CHECK(!t.has_value() || !t->defined() ||
                    (t->is_cuda() && t->scalar_type() == at::kFloat && t->numel() == C && t->is_contiguous()),
                "bn_forward_apply_gram: ", name, " must be a contiguous fp32 [C] GPU tensor");
  };
  check_c(weight, "weight");
  check_c(bias, "bias");
  check_c(running_mean, "running_mean");
  check_c(running_var, "running_var");
  TORCH_CHECK(gfptr(running_mean) == nullptr || gfptr(running_var) != nullptr, "running_var missing");
  int64_t* nbt = nullptr;
  if (num_batches_tracked.has_value() && num_batches_tracked->defined()) {
    TORCH_CHECK(num_batches_tracked->scalar_type() == at::kLong && num_batches_tracked->numel() == 1 &&
                    num_batches_tracked->is_cuda(), "num_batches_tracked must be a 1-element int64 GPU tensor");
    nbt = num_batches_tracked->data_ptr<int64_t>();
  }
  const int64_t M = x.numel() / C;
  auto y = at::empty_like(x);
  auto saved = at::empty({2, C}, x.options().dtype(at::kFloat));
  auto osums = at::empty({2 * C + 1}, x.options().dtype(at::kDouble));
  auto G = at::empty({C, C}, x.options().dtype(at::kFloat));
  TORCH_CHECK(M > 0, "bn_forward_apply_gram: empty input");
  // whole 64-row steps per block, ~target blocks
  const int target = gram_target_blocks((int)C);
  int64_t rows = (M + target - 1) / target;
  rows = (rows + kGStep - 1) / kGStep * kGStep;
  const int nb = (int)((M + rows - 1) / rows);
  auto opart = at::empty({2, (int64_t)nb, C}, x.options().dtype(at::kFloat));
  auto gpart = at::empty({(int64_t)nb, C, C}, x.options().dtype(at::kFloat));
  double* zt = moments_zero_target(osums.data_ptr<double>(), nb);
  auto stream = at::hip::getCurrentHIPStream();
  const bool nt = bn_streaming(M, C);
#define DMP_BN_GRAM(CC, NT)                                                                                  \
  hipLaunchKernelGGL((bn_apply_gram_kernel<CC, NT>), dim3(nb), dim3(kGThreads), 0, stream,                   \
                     reinterpret_cast<const bf16*>(x.data_ptr()), sums.data_ptr<double>(), gfptr(weight),    \
                     gfptr(bias), gfptr(running_mean), gfptr(running_var), (float)momentum, (float)eps, M,   \
                     rows, reinterpret_cast<bf16*>(y.data_ptr()), saved.data_ptr<float>(),                   \
                     saved.data_ptr<float>() + C, nbt, opart.data_ptr<float>(), zt, gpart.data_ptr<float>(), \
                     (float)clip)
#define DMP_BN_GRAM_C(CC) do { if (nt) DMP_BN_GRAM(CC, true); else DMP_BN_GRAM(CC, false); } while (0)
  if (C == 64) DMP_BN_GRAM_C(64);
  else if (C == 128) DMP_BN_GRAM_C(128);
  else DMP_BN_GRAM_C(256);
#undef DMP_BN_GRAM_C
#undef DMP_BN_GRAM
  DMP_HIP_CHECK(hipGetLastError());
  bn_reduce_partials_launch(opart.data_ptr<float>(), nb, (int)C, osums.data_ptr<double>(), (double)M, stream);
  split_reduce_launch(gpart.data_ptr<float>(), nb, C * C, G, stream);
  return {y, saved[0], saved[1], osums, G};
}

}  // namespace dmp
