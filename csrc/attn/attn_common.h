// Building blocks shared by the packed-qkv attention kernels (attention.hip:
// S <= 256, whole sequence in LDS; attention_long.hip: K / V and Q / dO
// streamed through LDS in chunks).  See attention.hip's header for the MFMA
// operand arrangement these helpers implement.
#pragma once

#include <torch/extension.h>
#include "../common.h"

namespace dmp {
namespace {

using bf16 = __bf16;
using v4i16 = short __attribute__((ext_vector_type(4)));
using lds_v4 = __attribute__((address_space(3))) v4i16;
constexpr int DH = 64;
constexpr int LROW = DH + 8;  // LDS row stride (bf16): 144 B, 16-B aligned rows, spreads banks
constexpr int kThreads = 256;
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ bf16x8 lds8(const bf16* base, int row, int col) {
  return *reinterpret_cast<const bf16x8*>(base + row * LROW + col);
}

// pi-ordered transposed read: lane (group g, index i) gets column col0 + i of
// rows rbase + 4g + {0..3} (elements 0-3) and rbase + 16 + 4g + {0..3} (4-7).
__device__ __forceinline__ bf16x8 lds_tr8(const bf16* base, int rbase, int col0, int lane) {
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;
  const bf16* a = base + (rbase + 4 * g + q) * LROW + col0 + 4 * p;
  v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)a);
  v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(a + 16 * LROW));
  short __attribute__((ext_vector_type(8))) t = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, t);
}

// two stacked D tiles -> one pi-ordered MFMA operand
__device__ __forceinline__ bf16x8 pack_pi(const float (&a)[4], const float (&b)[4]) {
  f32x8 f = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_convertvector(f, bf16x8);
}

// v_exp_f32 / v_log_f32 / v_rcp_f32 directly: exp2f / log2f / 1/x expand to
// 4-5 VALU each for denormal range handling (a compare, two selects and a
// v_ldexp around the v_exp), which the softmax never needs -- its exp2
// arguments are <= 0 (a tiny result flushing to 0 is the right answer), l >= 1
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float lg2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }

__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// rows [0, S) of two [S, 64] strided matrices into zero-padded [SP][LROW] LDS
// images.  Every global load of both images is issued before the first LDS
// store (SP*16/256 16-B loads in flight per lane instead of one): the staging
// is the latency-bound head of both kernels.
template <int SP, int NT = kThreads>
__device__ __forceinline__ void stage2(bf16* dst0, const bf16* src0, int64_t ld0, bf16* dst1,
                                       const bf16* src1, int64_t ld1, int S) {
  constexpr int PER = SP * (DH / 8);
  constexpr int IT = (PER + NT - 1) / NT;
  bf16x8 r0[IT], r1[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int v = threadIdx.x + i * NT;
    const int r = v >> 3, c = (v & 7) * 8;
    const bool ok = v < PER && r < S;
    r0[i] = ok ? *reinterpret_cast<const bf16x8*>(src0 + (int64_t)r * ld0 + c) : bf16x8{};
    r1[i] = ok ? *reinterpret_cast<const bf16x8*>(src1 + (int64_t)r * ld1 + c) : bf16x8{};
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int v = threadIdx.x + i * NT;
    if (v < PER) {
      const int r = v >> 3, c = (v & 7) * 8;
      *reinterpret_cast<bf16x8*>(dst0 + r * LROW + c) = r0[i];
      *reinterpret_cast<bf16x8*>(dst1 + r * LROW + c) = r1[i];
    }
  }
}

__device__ __forceinline__ void store4(bf16* p, const f32x4& v, float s) {
  bf16x4 o = {(bf16)(v[0] * s), (bf16)(v[1] * s), (bf16)(v[2] * s), (bf16)(v[3] * s)};
  *reinterpret_cast<bf16x4*>(p) = o;
}

inline void check_2d(const at::Tensor& t, const char* name, int64_t rows, int64_t min_cols) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.dim() == 2, name,
              " must be a 2-D bf16 GPU tensor");
  TORCH_CHECK(t.size(0) == rows && t.size(1) >= min_cols, name, " has the wrong shape");
  TORCH_CHECK(t.stride(1) == 1 && t.stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              name, " rows must be contiguous and 16-byte aligned");
}

}  // namespace

// ---- attention_long.hip: streamed kernels, called by attention.hip's entry points ----
constexpr int64_t kAttnLongMaxS = 4096;  // host-side cap; tested to S = 1025
inline int64_t attention_long_spl(int64_t S) { return (S + 63) / 64 * 64; }
std::vector<at::Tensor> attention_long_forward(const at::Tensor& qkv, int64_t B, int64_t S, int64_t H, double scale);
at::Tensor attention_long_backward(const at::Tensor& dout, const at::Tensor& qkv, const at::Tensor& o,
                                   const at::Tensor& lse, int64_t B, int64_t S, int64_t H, double scale);

}  // namespace dmp
