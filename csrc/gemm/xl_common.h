// What the large-tile NT kernels (gemm_xl_nt8.hip, gemm_xl_w4.hip,
// gemm_xl_x2.hip and their host file gemm_xl.hip, through xl_nt.h) and TN
// kernels (gemm_tn_xl.hip) share: the K tile and block size, the LDS-DMA copy,
// counted waits and the raw barrier, the implicit-GEMM conv view, the zero row
// of padding taps, the tied-accumulator MFMA of the 4-wave kernels and the
// operand check.  Everything but XlConv (a member of structs that cross
// translation units) is in an unnamed namespace: each source gets its own copy
// (g_zero_row included).
#pragma once

#include <torch/extension.h>
#include "../common.h"

namespace dmp {

// Implicit-GEMM convolution view of an operand (the 256 x 256 kernels only):
// GEMM row m is output pixel (n, oh, ow) of an NHWC input [N, Hi, Wi, cin]; K
// tile kt is channels c0..c0+63 of tap (tr, tc), K = taps * cin.  cin == 0:
// plain GEMM.
struct XlConv {
  int cin = 0, hi = 0, wi = 0, ho = 0, wo = 0, stride = 1, pad = 0, kw = 1;
};

namespace {

using bf16 = __bf16;
constexpr int XBK = 64, XTHREADS = 512;

using gptr_t = const __attribute__((address_space(1))) void*;
using lptr_t = __attribute__((address_space(3))) void*;

__device__ __forceinline__ void glds16(const void* g, char* l) {
  __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)l, 16, 0, 0);
}

template <int N>
__device__ __forceinline__ void vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ void barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// 16-B reads of padding taps land here (LDS-DMA cannot write zeros itself).
__device__ __attribute__((aligned(16))) bf16 g_zero_row[128] = {};

// MFMA of the 4-wave kernels (gemm_xl_w4_kernel, gemm_tn_w4_kernel: one wave
// per SIMD, 64 accumulators in all 256 AGPRs)
__device__ __forceinline__ void w4_mfma(f32x4& c, const bf16x8& a, const bf16x8& b) {
  // tied dst == srcC in AGPRs: the builtin lets the register allocator pick an
  // untied dst for some accumulators and rotate all 256 through v_accvgpr
  // moves every K tile; "memory" pins the order of the interleaved LDS reads /
  // copies.  srcA/B come from ds_read results the compiler waits for; the
  // accumulate chain D -> C needs no wait states; reads of the accumulators
  // after the loop sit behind w4_drain().
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b) : "memory");
}
__device__ __forceinline__ void w4_drain() { asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory"); }

inline void check_bf16_2d(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.dim() == 2, name,
              " must be a 2-D bf16 GPU tensor");
  TORCH_CHECK(t.stride(1) == 1 && t.stride(0) % 8 == 0, name, " rows must be contiguous and 16-B aligned");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-B aligned");
}

}  // namespace
}  // namespace dmp
