// Packed-qkv self-attention for sequences that do not fit one workgroup's LDS
// (S > 256: ViT-B/16 at 384 px has 577 tokens, ViT-B/8 at 224 px 785,
// ViT-B/16 at 512 px 1025), head dim 64, gfx950.  Same layout contract, MFMA
// operand arrangement and saved base-2 logsumexp as attention.hip; the
// building blocks live in attn_common.h.  The sequence is streamed through LDS
// in chunks of KC = 256 rows (2 images x 256 x 144 B = 72 KB, two workgroups
// per CU) instead of being held whole.
//
// Forward: one workgroup (4 waves x 2 query tiles) owns 128 queries of one
// (batch, head); the Q fragments and the O^T accumulators stay in registers,
// K / V chunks pass through LDS, the softmax is online (running max m and sum
// l per query, accumulator rescaled by exp2(m_old - m_new); P rounded to
// bf16).  A chunk is consumed in steps of 128 keys -- the scores of 256 do not
// fit the registers beside the accumulators -- and a tail of <= 64 keys runs
// the 64-key instantiation.
//
// Backward: a pre-pass writes D_i = rowsum(dO * O); then one workgroup per
// 64-row slice of a (batch, head), one 16-row tile per wave.  Phase A takes
// the slice as keys: dK^T / dV^T in registers, Q / dO (+ lse, D) chunks
// through LDS.  Phase B takes it as queries: dQ^T in registers, K / V chunks
// through LDS.  No atomics, nothing accumulated through memory: results are
// bitwise reproducible.
//
// Barriers sit inside the chunk loops, whose trip counts depend on S alone:
// every wave of a workgroup runs the same barriers.  Rows past S are clamped
// on load and masked on store; a wave whose rows all lie past S skips only
// the barrier-free compute of a chunk.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "../api.h"
#include "attn_common.h"

namespace dmp {
namespace {

constexpr int KC = 256;       // rows per LDS chunk
constexpr int FWD_QT = 2;     // query tiles per wave: each K / V fragment read feeds two MFMAs
constexpr int FWD_QB = 4 * FWD_QT * 16;  // queries per forward workgroup
constexpr int FWD_KS = 128;   // keys per online-softmax step: 2 x 8 score tiles in registers (a
                              // whole chunk's 2 x 16 spilled: 432 B/lane of scratch at 256 VGPRs)
constexpr int BWD_RB = 64;    // rows per backward workgroup (4 waves x one 16-row tile)

// one online-softmax step over NKT 16-key tiles of the chunk in LDS, `rows` keys of them real (rows >= 1)
template <int NKT, int QT>
__device__ __forceinline__ void fwd_chunk(const bf16* Ks, const bf16* Vs, const bf16x8 (&qf)[QT][2], int rows,
                                          float sl2, int lane, float (&m)[QT], float (&l)[QT],
                                          f32x4 (&acc)[QT][4]) {
  const int g = lane >> 4, li = lane & 15;
  f32x4 st[QT][NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    const bf16x8 k0 = lds8(Ks, kt * 16 + li, g * 8), k1 = lds8(Ks, kt * 16 + li, 32 + g * 8);
#pragma unroll
    for (int u = 0; u < QT; ++u) st[u][kt] = mfma(k1, qf[u][1], mfma(k0, qf[u][0], f32x4{0.f, 0.f, 0.f, 0.f}));
  }
  // padded keys -> -inf after the whole MFMA chain (as attention.hip)
  if (rows < NKT * 16) {
    int lim = rows - 4 * g;
    asm volatile("" : "+v"(lim));
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
      if (kt * 16 + 16 > rows) {  // uniform
#pragma unroll
        for (int u = 0; u < QT; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (kt * 16 + e >= lim) st[u][kt][e] = -INFINITY;
      }
  }
#pragma unroll
  for (int u = 0; u < QT; ++u) {
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int e = 0; e < 4; ++e) mx = fmaxf(mx, st[u][kt][e]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // the chunk holds a real key, so mn is finite; m = -inf before the first
    // chunk gives alpha = exp2(-inf) = 0 on a zero accumulator
    const float mn = fmaxf(m[u], mx * sl2);
    const float alpha = ex2(m[u] - mn);
    m[u] = mn;
    float ls = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = ex2(st[u][kt][e] * sl2 - mn);
        st[u][kt][e] = p;
        ls += p;
      }
    ls += __shfl_xor(ls, 16, 64);
    ls += __shfl_xor(ls, 32, 64);
    l[u] = l[u] * alpha + ls;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[u][t] *= alpha;
  }
#pragma unroll
  for (int kc = 0; kc < NKT / 2; ++kc) {
    bf16x8 pb[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) {
      float p0[4], p1[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { p0[e] = st[u][2 * kc][e]; p1[e] = st[u][2 * kc + 1][e]; }
      pb[u] = pack_pi(p0, p1);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bf16x8 vf = lds_tr8(Vs, kc * 32, t * 16, lane);
#pragma unroll
      for (int u = 0; u < QT; ++u) acc[u][t] = mfma(vf, pb[u], acc[u][t]);
    }
  }
}

// grid: (batch, head, 128-query block) in blockIdx.x
__global__ __launch_bounds__(kThreads, 2) void attn_long_fwd_kernel(const bf16* __restrict__ qkv, int64_t ld, int S,
                                                                  int H, int nqb, int SPL, float scale,
                                                                  bf16* __restrict__ o, int64_t ldo,
                                                                  float* __restrict__ lse) {
  constexpr int QT = FWD_QT;
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * KC * LROW];
  bf16* Ks = smem;
  bf16* Vs = smem + KC * LROW;
  // blocks of one (batch, head) share its K / V: keep them on one XCD's L2
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = bid / nqb, blk = bid - bh * nqb;
  const int b = bh / H, h = bh - b * H;
  const int D = H * DH;
  const bf16* qb = qkv + (int64_t)b * S * ld + h * DH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int q0 = blk * FWD_QB + wave * (QT * 16);
  const bool active = q0 < S;  // wave-uniform
  bf16x8 qf[QT][2];
#pragma unroll
  for (int u = 0; u < QT; ++u) {
    const int qc = min(q0 + u * 16 + li, S - 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      qf[u][ks] = *reinterpret_cast<const bf16x8*>(qb + (int64_t)qc * ld + ks * 32 + g * 8);
  }
  const float sl2 = scale * kLog2e;
  float m[QT], l[QT];
  f32x4 acc[QT][4];
#pragma unroll
  for (int u = 0; u < QT; ++u) {
    m[u] = -INFINITY;
    l[u] = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int c0 = 0; c0 < S; c0 += KC) {
    const int rows = min(KC, S - c0);
    __syncthreads();  // every wave finished reading the previous chunk
    {
      // two half-chunk passes (8 loads in flight per lane each): one pass of 16
      // beside the accumulators and Q fragments spills (44 B/lane of scratch)
      const bf16* kp = qb + D + (int64_t)c0 * ld;
      stage2<KC / 2>(Ks, kp, ld, Vs, kp + D, ld, rows);
      stage2<KC / 2>(Ks + KC / 2 * LROW, kp + (int64_t)(KC / 2) * ld, ld, Vs + KC / 2 * LROW,
                     kp + D + (int64_t)(KC / 2) * ld, ld, rows - KC / 2);
    }
    __syncthreads();
    if (active) {
#pragma unroll 1
      for (int k0 = 0; k0 < rows; k0 += FWD_KS) {  // uniform; every step holds a real key
        const int rs = min(FWD_KS, rows - k0);
        const bf16 *ks = Ks + k0 * LROW, *vs = Vs + k0 * LROW;
        if (rs <= FWD_KS / 2)
          fwd_chunk<FWD_KS / 32, QT>(ks, vs, qf, rs, sl2, lane, m, l, acc);
        else
          fwd_chunk<FWD_KS / 16, QT>(ks, vs, qf, rs, sl2, lane, m, l, acc);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < QT; ++u) {
    const int q = q0 + u * 16 + li;
    if (q < S) {
      const float inv = rcp(l[u]);
      bf16* orow = o + ((int64_t)b * S + q) * ldo + h * DH;
#pragma unroll
      for (int t = 0; t < 4; ++t) store4(orow + t * 16 + 4 * g, acc[u][t], inv);
      if (g == 0) lse[(int64_t)bh * SPL + q] = m[u] + lg2(l[u]);  // base-2 logsumexp of the scaled scores
    }
  }
}

// D[bh][s] = sum_d dO[t][h*64 + d] * O[t][h*64 + d], 8 lanes per (token, head) row
__global__ __launch_bounds__(kThreads) void attn_long_rowdot_kernel(const bf16* __restrict__ dout, int64_t ldd,
                                                                   const bf16* __restrict__ o, int64_t ldo,
                                                                   float* __restrict__ dd, int64_t nrows, int S,
                                                                   int H, int SPL) {
  const int64_t r = (int64_t)blockIdx.x * (kThreads / 8) + (threadIdx.x >> 3);
  const int64_t rc = r < nrows ? r : nrows - 1;
  const int64_t t = rc / H;
  const int h = (int)(rc - t * H);
  const int c = h * DH + (threadIdx.x & 7) * 8;
  const f32x8 x = __builtin_convertvector(*reinterpret_cast<const bf16x8*>(dout + t * ldd + c), f32x8);
  const f32x8 y = __builtin_convertvector(*reinterpret_cast<const bf16x8*>(o + t * ldo + c), f32x8);
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) a = fmaf(x[j], y[j], a);
  a += __shfl_xor(a, 1, 64);
  a += __shfl_xor(a, 2, 64);
  a += __shfl_xor(a, 4, 64);
  if (r < nrows && (threadIdx.x & 7) == 0) {
    const int64_t b = t / S;
    const int s = (int)(t - b * S);
    dd[(b * H + h) * SPL + s] = a;
  }
}

// grid: (batch, head, 64-row slice) in blockIdx.x
__global__ __launch_bounds__(kThreads, 2) void attn_long_bwd_kernel(
    const bf16* __restrict__ qkv, int64_t ld, const bf16* __restrict__ dout, int64_t ldd,
    const float* __restrict__ lse, const float* __restrict__ dd, int S, int H, int nsl, int SPL, float scale,
    bf16* __restrict__ dqkv, int64_t lddq) {
  // two LDS images, reused: Q / dO chunks in phase A, K / V chunks in phase B;
  // lse and D of the phase A chunk beside them.  72 KB + 2 KB -> 2 workgroups/CU.
  __shared__ __attribute__((aligned(16))) char smem[2 * KC * LROW * 2 + 2 * KC * 4];
  bf16* X0 = reinterpret_cast<bf16*>(smem);
  bf16* X1 = X0 + KC * LROW;
  float* lse_s = reinterpret_cast<float*>(X1 + KC * LROW);
  float* dd_s = lse_s + KC;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = bid / nsl, sl = bid - bh * nsl;
  const int b = bh / H, h = bh - b * H;
  const int D = H * DH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const float sl2 = scale * kLog2e;
  const bf16* qb = qkv + (int64_t)b * S * ld + h * DH;
  const bf16* db = dout + (int64_t)b * S * ldd + h * DH;
  bf16* dq_base = dqkv + (int64_t)b * S * lddq + h * DH;
  const float* lse_g = lse + (int64_t)bh * SPL;
  const float* dd_g = dd + (int64_t)bh * SPL;
  const int row0 = sl * BWD_RB + wave * 16;
  const bool active = row0 < S;  // wave-uniform
  const int row = row0 + li;     // this lane's key (phase A) / query (phase B)
  const int rowc = min(row, S - 1);

  // ---- phase A: the slice as keys; dV^T = dO^T P and dK^T = Q^T dS over all queries ----
  {
    bf16x8 kf[2], vf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kf[ks] = *reinterpret_cast<const bf16x8*>(qb + D + (int64_t)rowc * ld + ks * 32 + g * 8);
      vf[ks] = *reinterpret_cast<const bf16x8*>(qb + 2 * D + (int64_t)rowc * ld + ks * 32 + g * 8);
    }
    const float km = row < S ? 1.f : 0.f;
    f32x4 dv[4], dk[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { dv[t] = f32x4{0.f, 0.f, 0.f, 0.f}; dk[t] = dv[t]; }
    for (int c0 = 0; c0 < S; c0 += KC) {
      const int rows = min(KC, S - c0);
      __syncthreads();  // every wave finished reading the previous chunk
      stage2<KC>(X0, qb + (int64_t)c0 * ld, ld, X1, db + (int64_t)c0 * ldd, ldd, rows);  // Q, dO
      for (int r = threadIdx.x; r < KC; r += kThreads) {
        // a padded query's Q and dO rows are zero; lse = +inf makes its P zero as well
        lse_s[r] = r < rows ? lse_g[c0 + r] : INFINITY;
        dd_s[r] = r < rows ? dd_g[c0 + r] : 0.f;
      }
      __syncthreads();
      if (active) {
        const int nq = (rows + 31) >> 5;
#pragma unroll 1
        for (int qc = 0; qc < nq; ++qc) {
          float pp[2][4], dss[2][4];
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            const int q0 = qc * 32 + hf * 16;
            f32x4 sv = {0.f, 0.f, 0.f, 0.f}, dp = sv;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
              sv = mfma(lds8(X0, q0 + li, ks * 32 + g * 8), kf[ks], sv);
              dp = mfma(lds8(X1, q0 + li, ks * 32 + g * 8), vf[ks], dp);
            }
            const f32x4 ls = *reinterpret_cast<const f32x4*>(lse_s + q0 + 4 * g);
            const f32x4 dr = *reinterpret_cast<const f32x4*>(dd_s + q0 + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float pv = ex2(sv[e] * sl2 - ls[e]) * km;  // a multiply, not a branch around the exp
              pp[hf][e] = pv;
              dss[hf][e] = pv * (dp[e] - dr[e]);
            }
          }
          const bf16x8 pb = pack_pi(pp[0], pp[1]);
          const bf16x8 dsb = pack_pi(dss[0], dss[1]);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            dv[t] = mfma(lds_tr8(X1, qc * 32, t * 16, lane), pb, dv[t]);
            dk[t] = mfma(lds_tr8(X0, qc * 32, t * 16, lane), dsb, dk[t]);
          }
        }
      }
    }
    if (row < S) {
      bf16* out = dq_base + (int64_t)row * lddq;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        store4(out + D + t * 16 + 4 * g, dk[t], scale);
        store4(out + 2 * D + t * 16 + 4 * g, dv[t], 1.f);
      }
    }
  }

  // ---- phase B: the slice as queries; dQ^T = K^T dS^T over all keys ----
  {
    bf16x8 qf[2], dof[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[ks] = *reinterpret_cast<const bf16x8*>(qb + (int64_t)rowc * ld + ks * 32 + g * 8);
      dof[ks] = *reinterpret_cast<const bf16x8*>(db + (int64_t)rowc * ldd + ks * 32 + g * 8);
    }
    const float lq = lse_g[rowc], dq_d = dd_g[rowc];
    f32x4 dq[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < S; c0 += KC) {
      const int rows = min(KC, S - c0);
      __syncthreads();  // phase A / the previous chunk is done with X0 / X1
      stage2<KC>(X0, qb + D + (int64_t)c0 * ld, ld, X1, qb + 2 * D + (int64_t)c0 * ld, ld, rows);  // K, V
      __syncthreads();
      if (active) {
        const int nk = (rows + 31) >> 5;
#pragma unroll 1
        for (int kc = 0; kc < nk; ++kc) {
          float dss[2][4];
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            const int k0 = kc * 32 + hf * 16;
            f32x4 sv = {0.f, 0.f, 0.f, 0.f}, dp = sv;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
              sv = mfma(lds8(X0, k0 + li, ks * 32 + g * 8), qf[ks], sv);
              dp = mfma(lds8(X1, k0 + li, ks * 32 + g * 8), dof[ks], dp);
            }
            // no key mask: a padded key's K and V rows are zero in LDS, so its dS
            // multiplies a zero K row into dQ; the clamp keeps that dS finite
#pragma unroll
            for (int e = 0; e < 4; ++e) dss[hf][e] = ex2(fminf(sv[e] * sl2 - lq, 0.f)) * (dp[e] - dq_d);
          }
          const bf16x8 dsb = pack_pi(dss[0], dss[1]);
#pragma unroll
          for (int t = 0; t < 4; ++t) dq[t] = mfma(lds_tr8(X0, kc * 32, t * 16, lane), dsb, dq[t]);
        }
      }
    }
    if (row < S) {
      bf16* out = dq_base + (int64_t)row * lddq;
#pragma unroll
      for (int t = 0; t < 4; ++t) store4(out + t * 16 + 4 * g, dq[t], scale);
    }
  }
}

}  // namespace

// qkv [B*S, >= 3*H*64] -> (o [B*S, H*64], lse [B*H, SPL] fp32, base-2), SPL = S rounded up to 64
std::vector<at::Tensor> attention_long_forward(const at::Tensor& qkv, int64_t B, int64_t S, int64_t H,
                                               double scale) {
  const int64_t spl = attention_long_spl(S);
  const int64_t nqb = (S + FWD_QB - 1) / FWD_QB;
  TORCH_CHECK(B * H * nqb < (int64_t)1 << 31, "attention: too many (batch, head, query block) workgroups");
  auto o = at::empty({B * S, H * DH}, qkv.options());
  auto lse = at::empty({B * H, spl}, qkv.options().dtype(at::kFloat));
  if (B * H == 0) return {o, lse};
  hipStream_t st = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(attn_long_fwd_kernel, dim3(B * H * nqb), dim3(kThreads), 0, st, (const bf16*)qkv.data_ptr(),
                     qkv.stride(0), (int)S, (int)H, (int)nqb, (int)spl, (float)scale, (bf16*)o.data_ptr(),
                     o.stride(0), lse.data_ptr<float>());
  DMP_HIP_CHECK(hipGetLastError());
  return {o, lse};
}

at::Tensor attention_long_backward(const at::Tensor& dout, const at::Tensor& qkv, const at::Tensor& o,
                                   const at::Tensor& lse, int64_t B, int64_t S, int64_t H, double scale) {
  const int64_t spl = attention_long_spl(S);
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat && lse.is_contiguous() && lse.size(0) == B * H &&
                  lse.size(1) == spl, "attention: lse shape");
  const int64_t nsl = (S + BWD_RB - 1) / BWD_RB;
  TORCH_CHECK(B * H * nsl < (int64_t)1 << 31, "attention: too many (batch, head, slice) workgroups");
  auto dqkv = at::empty({B * S, 3 * H * DH}, qkv.options());
  if (B * H == 0) return dqkv;
  auto dd = at::empty({B * H, spl}, lse.options());
  hipStream_t st = at::hip::getCurrentHIPStream();
  const int64_t nrows = B * S * H;
  hipLaunchKernelGGL(attn_long_rowdot_kernel, dim3((nrows + kThreads / 8 - 1) / (kThreads / 8)), dim3(kThreads), 0,
                     st, (const bf16*)dout.data_ptr(), dout.stride(0), (const bf16*)o.data_ptr(), o.stride(0),
                     dd.data_ptr<float>(), nrows, (int)S, (int)H, (int)spl);
  DMP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(attn_long_bwd_kernel, dim3(B * H * nsl), dim3(kThreads), 0, st, (const bf16*)qkv.data_ptr(),
                     qkv.stride(0), (const bf16*)dout.data_ptr(), dout.stride(0), lse.data_ptr<float>(),
                     dd.data_ptr<float>(), (int)S, (int)H, (int)nsl, (int)spl, (float)scale,
                     (bf16*)dqkv.data_ptr(), dqkv.stride(0));
  DMP_HIP_CHECK(hipGetLastError());
  return dqkv;
}

}  // namespace dmp
