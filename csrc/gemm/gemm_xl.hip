// Large-tile MFMA bf16 NT GEMMs with fused epilogues: the transformer linears
// (ViT-B/16 qkv / proj / fc1 / fc2 in forward and data-gradient form) and the
// wide conv GEMMs of ResNet-50 (1x1 convs, and 3x3 / strided-dgrad convs as an
// implicit GEMM through the tap gather).
//
//   C[M, N] = epi( A[M, K] * B[N, K]^T )        (both operands K-contiguous)
//
// This file is the host side: the tile and main-loop policy, the five entry
// points, and the one route from a launch to a kernel (xl_launch).  The
// kernels, one per file, each behind one launcher:
//   gemm_xl_w4.hip   gemm_xl_w4_kernel  4 waves, 256 x 256 / 224 x 256 / 256 x
//                    128 tiles (PIPE 11, the default main loop of the 256-wide
//                    tiles)
//   gemm_xl_nt8.hip  gemm_xl_nt_kernel  8 waves: PIPE 10 = 256 x 256 ping-pong
//                    quadrants (the operand-heavy conv epilogues;
//                    DMP_XL_PIPE=10), PIPE 1 / 0 = the ring and two-buffer
//                    loops (256 x 128 tiles and A/B options)
//   gemm_xl_x2.hip   gemm_x2_kernel     256 x 128 tiles at two blocks per CU
//                    (conv epilogues, N = 128 + 256 j)
// Epilogues, arguments and the epilogue the first two share: xl_nt.h.  The TN
// (weight-gradient) kernels are in gemm_tn_xl.hip; what both sides use is in
// xl_common.h.
//
// Forward of nn.Linear: A = x [T, in], B = W [out, in].  Data gradient:
// A = dy [T, out], B = W^T [in, out] (a 4.7 MB transposed copy of W per step).
#include <cmath>
#include <cstdlib>
#include <ATen/hip/HIPContext.h>
#include "../api.h"
#include "../launch.h"
#include "xl_nt.h"

namespace dmp {
namespace {

int g_num_cus = 0;

// main loop of the 256 x 256 tiles: 11 = the 4-wave kernel (default), 10 =
// the 8-wave ping-pong quadrant schedule; 128-wide tiles run the half-step
// ring (1) or the round-1 two-buffer loop (0).  Measured and removed in round
// 6 (notes in profiles/README.md): the round-4 ping-pong that re-read B's n
// half 0 (7), its 10-slot LDS unit ring (8, slower: finding 43), the split-K
// tail (9, no faster: finding 54), the persistent form (6, slower: finding
// 66), timing-only ablations (2-5) and the non-temporal epilogue switch.
constexpr int kXlPipeDefault = 11;
int g_xl_pipe = [] {  // DMP_XL_PIPE=<n>: A/B of the main loop (10 = 8-wave ping-pong)
  const char* e = std::getenv("DMP_XL_PIPE");
  return e ? std::atoi(e) : kXlPipeDefault;
}();

int num_cus() {
  if (g_num_cus == 0) {
    int dev = 0;
    DMP_HIP_CHECK(hipGetDevice(&dev));
    DMP_HIP_CHECK(hipDeviceGetAttribute(&g_num_cus, hipDeviceAttributeMultiprocessorCount, dev));
  }
  return g_num_cus;
}

// Rows per tile of the PIPE 10 kernel.  One 256 x 256 block per CU makes a
// partly filled last round cost a full one (finding 54: layer-3 3x3s at batch
// 2048 are 1568 tiles = 6.1 rounds, ViT's N = 768 GEMMs 591 tiles = 2.3).
// An MFMA-bound GEMM (K >= 768) instead takes the tile height in
// {256, 240, .., 192} that minimises rounds x height: the skipped rows of a
// trimmed tile cost their staging only.  0 = auto, -1 = always 256, else forced (A/B).
int g_xl_bm = 0;

// rounds x rows of 1-block/CU work of an M x N GEMM in bm-row, 256-wide tiles
int64_t tile_rows_cost(int64_t M, int64_t N, int64_t bm) {
  const int64_t cus = num_cus(), nt = (N + 255) / 256;
  return ((M + bm - 1) / bm * nt + cus - 1) / cus * bm;
}

// 4-wave kernel (PIPE 11): 256- or 224-row tiles (MB = 8 / 7 blocks per
// wave), whichever needs fewer rounds x rows of 1-block/CU work: ViT's N = 768
// GEMMs 591 tiles (3 rounds x 256) -> 678 (3 x 224); ResNet-50 layer-3 3x3s
// 1568 (7 x 256) -> 1792 (7 x 224), layer-4 784 (4 x 256) -> 896 (4 x 224).
int pick_bm_w4(int64_t M, int64_t N) {
  if (N <= 128) return 256;  // the 256 x 128 tile (WN = 1) has 256 rows only
  if (g_xl_bm == 224 || g_xl_bm == 256) return g_xl_bm;
  if (g_xl_bm < 0) return 256;
  // a 12.5 % cut (whole rounds of 7/8 the rows) only: a tile's fixed cost
  // (prologue, epilogue) does not shrink with its rows, and ViT's fc1 forward
  // (N = 3072, K = 768: 10 rounds x 256 vs 11 x 224) measured 0.330 vs 0.339 ms
  return tile_rows_cost(M, N, 224) * 100 <= tile_rows_cost(M, N, 256) * 90 ? 224 : 256;
}

// the heavy-epilogue GEMMs the 4-wave default leaves on PIPE 10 (folded-BN
// affine, BN backward) are short-K: their tile time is mostly the epilogue,
// which scales with the tile's rows, so trimmed tiles pay there too
// (set_gemm_xl_trim_heavy, A/B)
int g_xl_trim_heavy = 1;

int pick_bm(int64_t M, int64_t N, int64_t K, int epi) {
  if (g_xl_pipe == 11 && w4_epi(epi)) return pick_bm_w4(M, N);
  const bool heavy = g_xl_pipe == 11 && g_xl_trim_heavy;
  if (g_xl_pipe != 10 && !heavy) return 256;
  if (g_xl_bm > 0) return g_xl_bm;
  if (g_xl_bm < 0 || (K < 768 && !heavy)) return 256;
  int best = 256;
  int64_t best_cost = tile_rows_cost(M, N, 256);
  for (int bm = 240; bm >= 192; bm -= 16) {
    const int64_t cost = tile_rows_cost(M, N, bm);
    if (cost * 100 < best_cost * 97) { best = bm; best_cost = cost; }
  }
  return best;
}

unsigned long long* g_xl_tdbg = nullptr;  // set_gemm_xl_trace

// the 4-wave kernel addresses A (plain) and B through 32-bit buffer offsets
bool w4_ok(const XlArgs& a) {
  const int64_t lim = (int64_t)1 << 31;
  const bool bfit = ((int64_t)(a.N - 1) * a.ldb + a.K) * 2 < lim;
  const bool afit = a.cv.cin > 0 || ((int64_t)(a.M - 1) * a.lda + (a.A2 ? a.K1 : a.K)) * 2 < lim;
  return bfit && afit;
}

// two-blocks-per-CU kernel (gemm_x2_kernel): 0 = off, 1 = where it measured
// faster than this kernel's 256 x 128 tile (N = 128 + 256 j: 1.14-1.59x on
// ResNet-50 l2 conv1 at batch 256, profiles/raw_r4/x2_bench_r4d.md; on
// N % 256 == 0 the 256 x 256 tile wins 0.76-1.08x), 2 = every conv-epilogue
// GEMM with N % 128 == 0 (A/B)
int g_xl_x2 = 1;

// (conv epilogues of a plain GEMM only: the implicit-GEMM gather has no x2 form)
bool use_x2(const XlArgs& a, int epi) {
  if (is_linear_epi(epi) || a.cv.cin > 0) return false;
  if (g_xl_x2 == 0 || a.N % X2_BN != 0) return false;
  return g_xl_x2 == 2 || a.N % 256 != 0;
}

int g_xl_bn_override = 0;
int g_xl_group_m = 0;

// BN choice: 256-wide tiles unless that leaves the last round of a 1-block/CU
// grid mostly empty (N = 768: 3 column tiles -> 128-wide gives 2x the blocks).
int pick_bn(int M, int N) {
  if (g_xl_bn_override) return g_xl_bn_override;
  if (g_xl_pipe == 11) return 256;  // the 4-wave kernel has 256-wide tiles only
  const int cus = 256;
  auto eff = [&](int bn) {
    const double blocks = (double)((M + XBM - 1) / XBM) * ((N + bn - 1) / bn);
    const double rounds = std::ceil(blocks / cus);
    // useful work / (rounds x tile work); the 128-wide tile runs the ring
    // loop, ~12 % slower per FLOP than the 256-wide ring and ~25 % slower than
    // the 256-wide ping-pong loop (profiles/vit_gemm_backends.md)
    return blocks / (rounds * cus) * (bn == 256 ? 1.0 : (g_xl_pipe >= 10 ? 0.75 : 0.88));
  };
  return eff(128) > eff(256) ? 128 : 256;
}

// The one route from a launch to a kernel.  a.bm came from pick_bm (the
// moments partials are sized by it) and is 256 where use_x2 holds.  In order:
// the two-blocks-per-CU kernel; 128-wide tiles (ring / two-buffer loop only);
// 256-wide tiles under PIPE 10 / 11, and every implicit-GEMM conv (those are
// the only main loops with the tap gather) -- the 4-wave kernel where it takes
// the epilogue and the operands fit its 32-bit offsets, else the 8-wave
// ping-pong; 256-wide ring / two-buffer loop.  The conv epilogues have no
// two-buffer (PIPE 0) form and run the ring there.  Tracing (set_gemm_xl_trace)
// covers the PIPE 10 / 11 launches.
void xl_launch(XlArgs a, int epi, int bn, hipStream_t s) {
  if (use_x2(a, epi)) return launch_xl_x2(a, epi, s);
  const int tbm = (bn == 256 && a.bm > 0) ? a.bm : XBM;
  const int blocks = ((a.M + tbm - 1) / tbm) * ((a.N + bn - 1) / bn);
  const int ring = (g_xl_pipe == 0 && is_linear_epi(epi)) ? 0 : 1;
  if (bn == 128) return launch_xl_nt8(a, epi, 128, ring, blocks, s);
  if (g_xl_pipe >= 10 || a.cv.cin > 0) {
    a.tdbg = g_xl_tdbg;
    if (g_xl_pipe == 11 && w4_epi(epi) && w4_ok(a)) return launch_xl_w4(a, epi, s);
    return launch_xl_nt8(a, epi, 256, 10, blocks, s);
  }
  launch_xl_nt8(a, epi, 256, ring, blocks, s);
}

const bf16* bf16_ptr(const at::Tensor& t) { return reinterpret_cast<const bf16*>(t.data_ptr()); }
bool given(const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); }

// The operands of one launch: A (rows of lda elements: a conv's A is the NHWC
// image, one row per pixel), B, C if it exists yet, the GEMM sizes and the
// tile-order group.
XlArgs xl_operands(const at::Tensor& A, int64_t lda, const at::Tensor& B, int64_t M, int64_t N, int64_t K,
                   const at::Tensor& C = at::Tensor()) {
  XlArgs a{};
  a.A = bf16_ptr(A); a.lda = lda;
  a.B = bf16_ptr(B); a.ldb = B.stride(0);
  if (C.defined()) { a.C = const_cast<bf16*>(bf16_ptr(C)); a.ldc = C.stride(0); }
  a.M = (int)M; a.N = (int)N; a.K = (int)K;
  a.group_m = g_xl_group_m > 0 ? g_xl_group_m : 4;
  return a;
}

XlConv xl_conv_geom(int64_t cin, int64_t hi, int64_t wi, int64_t ho, int64_t wo, int64_t stride, int64_t pad,
                    int64_t kw) {
  XlConv cv;
  cv.cin = (int)cin; cv.hi = (int)hi; cv.wi = (int)wi; cv.ho = (int)ho; cv.wo = (int)wo;
  cv.stride = (int)stride; cv.pad = (int)pad; cv.kw = (int)kw;
  return cv;
}

// mode string -> epilogue, among the epilogues in `accept` (bit e: XlEpi e)
constexpr unsigned epi_bit(int e) { return 1u << e; }
int xl_mode(const std::string& mode, unsigned accept, const char* who) {
  static const struct { const char* name; int epi; } kModes[] = {
      {"store", XL_STORE}, {"bias", XL_BIAS}, {"bias_gelu", XL_BIAS_GELU}, {"dgelu", XL_DGELU},
      {"bias_res", XL_BIAS_RES}, {"bias_res_scale", XL_BIAS_RES_SCALE}, {"moments", XL_MOMENTS}, {"add", XL_ADD}, {"bnbwd", XL_BNBWD},
      {"affine", XL_AFFINE}};
  int epi = -1;
  for (const auto& m : kModes)
    if (mode == m.name && (accept & epi_bit(m.epi))) epi = m.epi;
  TORCH_CHECK(epi >= 0, who, ": unknown mode ", mode);
  return epi;
}

}  // namespace

// C = epi(A @ B^T).  mode: "store" | "bias" | "bias_gelu" | "dgelu" | "bias_res" |
// "bias_res_scale" (bias_res with the branch scaled per sample: row m takes
// row_scale[m / rows_per_sample]).
// Returns C ("bias_gelu": also fills aux with the pre-activation).
at::Tensor gemm_xl(const at::Tensor& A, const at::Tensor& B, const std::string& mode,
                   const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& aux,
                   const c10::optional<at::Tensor>& residual, const c10::optional<at::Tensor>& out,
                   const c10::optional<at::Tensor>& row_scale, int64_t rows_per_sample) {
  check_bf16_2d(A, "A");
  check_bf16_2d(B, "B");
  const int64_t M = A.size(0), K = A.size(1), N = B.size(0);
  TORCH_CHECK(B.size(1) == K, "gemm_xl: A/B K mismatch");
  TORCH_CHECK(K % XBK == 0 && K >= XBK, "gemm_xl: K must be a positive multiple of 64");
  TORCH_CHECK(N % 8 == 0, "gemm_xl: N must be a multiple of 8");
  TORCH_CHECK(M > 0 && M < (1LL << 31) && N < (1LL << 31), "gemm_xl: size out of range");
  TORCH_CHECK(A.device() == B.device(), "gemm_xl: device mismatch");
  const int epi = xl_mode(mode, epi_bit(XL_STORE) | epi_bit(XL_BIAS) | epi_bit(XL_BIAS_GELU) | epi_bit(XL_DGELU) |
                                    epi_bit(XL_BIAS_RES) | epi_bit(XL_BIAS_RES_SCALE), "gemm_xl");
  at::Tensor C;
  if (out) {
    C = *out;
    check_bf16_2d(C, "out");
    TORCH_CHECK(C.size(0) == M && C.size(1) == N, "gemm_xl: out shape");
  } else {
    C = at::empty({M, N}, A.options());
  }
  XlArgs a = xl_operands(A, A.stride(0), B, M, N, K, C);
  if (epi == XL_BIAS || epi == XL_BIAS_GELU || epi == XL_BIAS_RES || epi == XL_BIAS_RES_SCALE) {
    TORCH_CHECK(bias && bias->scalar_type() == at::kBFloat16 && bias->numel() == N && bias->is_contiguous(),
                "gemm_xl: bias must be a contiguous bf16 [N]");
    a.bias = bf16_ptr(*bias);
  }
  if (epi == XL_BIAS_GELU || epi == XL_DGELU) {
    TORCH_CHECK(aux.has_value(), "gemm_xl: mode needs aux");
    check_bf16_2d(*aux, "aux");
    TORCH_CHECK(aux->size(0) == M && aux->size(1) == N, "gemm_xl: aux shape");
    a.aux = const_cast<bf16*>(bf16_ptr(*aux));
    a.ldaux = aux->stride(0);
  }
  if (epi == XL_BIAS_RES || epi == XL_BIAS_RES_SCALE) {
    TORCH_CHECK(residual.has_value(), "gemm_xl: ", mode, " needs residual");
    check_bf16_2d(*residual, "residual");
    TORCH_CHECK(residual->size(0) == M && residual->size(1) == N, "gemm_xl: residual shape");
    a.R = bf16_ptr(*residual);
    a.ldr = residual->stride(0);
  }
  if (epi == XL_BIAS_RES_SCALE) {
    TORCH_CHECK(given(row_scale) && row_scale->is_cuda() && row_scale->device() == A.device() &&
                    row_scale->scalar_type() == at::kFloat && row_scale->is_contiguous(),
                "gemm_xl: row_scale must be a contiguous fp32 tensor on A's device");
    TORCH_CHECK(rows_per_sample > 0, "gemm_xl: rows_per_sample must be positive");
    TORCH_CHECK(row_scale->numel() * rows_per_sample == M, "gemm_xl: M (", M, ") must be row_scale.numel() (",
                row_scale->numel(), ") * rows_per_sample (", rows_per_sample, ")");
    a.rscale = row_scale->data_ptr<float>();
    a.rows_per_sample = (int)rows_per_sample;
  } else {
    TORCH_CHECK(!given(row_scale), "gemm_xl: row_scale is for mode bias_res_scale only");
  }
  const int bn = pick_bn((int)M, (int)N);
  a.bm = bn == 256 ? pick_bm(M, N, K, epi) : 256;
  xl_launch(a, epi, bn, at::hip::getCurrentHIPStream());
  DMP_HIP_CHECK(hipGetLastError());
  return C;
}

// dh = bf16(bf16(A @ B^T) * gelu'(aux)) (fc2's data gradient through the GELU)
// and fc1's bias gradient sum_rows dh (fp32 [N]) from the same epilogue: the
// column sums leave as per-M-tile partials, no separate pass over dh.
std::vector<at::Tensor> gemm_xl_dgelu_bgrad(const at::Tensor& A, const at::Tensor& B, const at::Tensor& aux) {
  check_bf16_2d(A, "A");
  check_bf16_2d(B, "B");
  check_bf16_2d(aux, "aux");
  const int64_t M = A.size(0), K = A.size(1), N = B.size(0);
  TORCH_CHECK(B.size(1) == K && K % XBK == 0 && K >= XBK && N % 8 == 0, "gemm_xl_dgelu_bgrad: shapes");
  TORCH_CHECK(M > 0 && M < (1LL << 31), "gemm_xl_dgelu_bgrad: M out of range");
  TORCH_CHECK(aux.size(0) == M && aux.size(1) == N, "gemm_xl_dgelu_bgrad: aux shape");
  auto C = at::empty({M, N}, A.options());
  XlArgs a = xl_operands(A, A.stride(0), B, M, N, K, C);
  a.aux = const_cast<bf16*>(bf16_ptr(aux)); a.ldaux = aux.stride(0);
  const int bn = pick_bn((int)M, (int)N);
  a.bm = bn == 256 ? pick_bm(M, N, K, XL_DGELU) : 256;
  const int mtiles = (int)((M + a.bm - 1) / a.bm);
  auto part = at::empty({2, mtiles, N}, A.options().dtype(at::kFloat));
  a.part = part.data_ptr<float>();
  xl_launch(a, XL_DGELU, bn, at::hip::getCurrentHIPStream());
  DMP_HIP_CHECK(hipGetLastError());
  return {C, part[0].sum(0)};
}

// Wide 1x1-conv GEMMs with the conv epilogues on the glds-ring kernel:
//   "moments": C = bf16(A @ B^T), returns fp64 [2N+1] (sum, sum^2, M) of C
//   "add"    : C = bf16(bf16(A @ B^T) + residual)
//   "bnbwd"  : C = dz = mask * bf16(A @ B^T (+ residual)), returns (sum dz, sum dz*(x-mean), M)
//              (same contract as gemm_nt_bnbwd)
//   "affine" : C = act(A @ B^T * scale + shift (+ residual))
namespace {

// Epilogue operands of the conv epilogues (absent: nullopt or undefined)
struct XlConvEpi {
  c10::optional<at::Tensor> residual;                   // add / affine / bnbwd
  c10::optional<at::Tensor> bn_x, bn_y;                 // bnbwd: BN input / output (mask source)
  c10::optional<at::Tensor> mean, invstd, weight, bias; // bnbwd: BN statistics and affine, fp32 [N]
  c10::optional<at::Tensor> ebias;                      // bnbwd: per-column constant, fp32 [N]
  c10::optional<at::Tensor> scale, shift;               // affine coefficients, fp32 [N] (absent: 1 / 0)
  bool relu = false;                                    // affine
  std::vector<int64_t> res_map;                         // bnbwd: compact residual [stride, Ho, Wo, Hi, Wi]
};

// Shared tail of gemm_xl_conv / conv_xl: epilogue operands, launch, moments reduce.
// `a` holds the operands and M, N, K; conv (a.cv.cin > 0) always runs a
// 256-wide PIPE 10 / 11 kernel (the only main loops with the gather).
std::vector<at::Tensor> xl_conv_run(XlArgs a, const at::Tensor& A, const std::string& mode, const XlConvEpi& e) {
  const int64_t M = a.M, N = a.N;
  const bool conv = a.cv.cin > 0;
  int epi = xl_mode(mode, epi_bit(XL_MOMENTS) | epi_bit(XL_ADD) | epi_bit(XL_BNBWD) | epi_bit(XL_AFFINE) |
                              (conv ? epi_bit(XL_STORE) : 0u), "gemm_xl_conv");
  TORCH_CHECK(!conv || epi != XL_AFFINE, "conv_xl: mode ", mode, " has no implicit-GEMM variant");
  auto C = at::empty({M, N}, A.options());
  a.C = reinterpret_cast<bf16*>(C.data_ptr()); a.ldc = C.stride(0);
  if (!e.res_map.empty()) {
    TORCH_CHECK(mode == "bnbwd" && e.res_map.size() == 5, "res_map: bnbwd only, [stride, Ho, Wo, Hi, Wi]");
    a.rmap.s = (int)e.res_map[0]; a.rmap.ho = (int)e.res_map[1]; a.rmap.wo = (int)e.res_map[2];
    a.rmap.hi = (int)e.res_map[3]; a.rmap.wi = (int)e.res_map[4];
    TORCH_CHECK(a.rmap.ho == (a.rmap.hi + a.rmap.s - 1) / a.rmap.s &&
                    a.rmap.wo == (a.rmap.wi + a.rmap.s - 1) / a.rmap.s && M % ((int64_t)a.rmap.hi * a.rmap.wi) == 0,
                "res_map does not describe a stride-s subsampling of the GEMM rows");
  }
  if (given(e.residual)) {
    check_bf16_2d(*e.residual, "residual");
    const int64_t rrows = a.rmap.s == 1 ? M : M / ((int64_t)a.rmap.hi * a.rmap.wi) * a.rmap.ho * a.rmap.wo;
    TORCH_CHECK(e.residual->size(0) == rrows && e.residual->size(1) == N, "gemm_xl_conv: residual shape");
    a.R = bf16_ptr(*e.residual);
    a.ldr = e.residual->stride(0);
  }
  TORCH_CHECK(epi != XL_ADD || a.R, "gemm_xl_conv: add needs a residual");
  auto f32vec = [&](const c10::optional<at::Tensor>& t, const char* name) {
    TORCH_CHECK(t.has_value() && t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() &&
                    t->numel() == N && reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                name, " must be a contiguous 16-B aligned fp32 [N] GPU tensor");
    return t->data_ptr<float>();
  };
  if (epi == XL_AFFINE) {
    if (given(e.scale)) a.esc = f32vec(e.scale, "scale");
    if (given(e.shift)) a.esh = f32vec(e.shift, "shift");
    a.erelu = e.relu;
  }
  if (epi == XL_BNBWD) {
    const bool has_x = given(e.bn_x), has_y = given(e.bn_y);
    epi = !has_y ? XL_BNBWD : has_x ? XL_BNBWD_Y : XL_BNBWD_YO;
    TORCH_CHECK(has_x || has_y, "bnbwd needs bn_x and/or bn_y");
    if (has_x) {
      check_bf16_2d(*e.bn_x, "bn_x");
      TORCH_CHECK(e.bn_x->size(0) == M && e.bn_x->size(1) == N, "bn_x shape");
      a.bx = bf16_ptr(*e.bn_x); a.ldbx = e.bn_x->stride(0);
      a.bmean = f32vec(e.mean, "mean");
    }
    if (given(e.ebias)) a.ebias = f32vec(e.ebias, "ebias");
    if (has_y) {
      check_bf16_2d(*e.bn_y, "bn_y");
      TORCH_CHECK(e.bn_y->size(0) == M && e.bn_y->size(1) == N, "bn_y shape");
      a.bny = bf16_ptr(*e.bn_y); a.ldby = e.bn_y->stride(0);
    } else {
      a.binv = f32vec(e.invstd, "invstd");
      if (given(e.weight)) a.bw = f32vec(e.weight, "weight");
      if (given(e.bias)) a.bb = f32vec(e.bias, "bias");
    }
  }
  const int bn = conv ? 256 : pick_bn((int)M, (int)N);
  // the two-blocks-per-CU route keeps 256-row tiles
  a.bm = (bn == 256 && !use_x2(a, epi)) ? pick_bm(M, N, a.K, epi) : 256;
  at::Tensor sums, part;
  const int mtiles = (int)((M + a.bm - 1) / a.bm);
  const bool moments = epi == XL_MOMENTS || is_bnbwd(epi);
  if (moments) {
    part = at::empty({2, mtiles, N}, A.options().dtype(at::kFloat));
    sums = at::empty({2 * N + 1}, A.options().dtype(at::kDouble));
    a.part = part.data_ptr<float>();
    a.zsums = moments_zero_target(sums.data_ptr<double>(), mtiles);
  }
  hipStream_t s = at::hip::getCurrentHIPStream();
  xl_launch(a, epi, bn, s);
  DMP_HIP_CHECK(hipGetLastError());
  if (moments) bn_reduce_partials_launch(a.part, mtiles, (int)N, sums.data_ptr<double>(), (double)M, s);
  return {C, sums};
}

}  // namespace

std::vector<at::Tensor> gemm_xl_conv(const at::Tensor& A, const at::Tensor& B, const std::string& mode,
                                     const c10::optional<at::Tensor>& residual,
                                     const c10::optional<at::Tensor>& bn_x,
                                     const c10::optional<at::Tensor>& bn_y,
                                     const c10::optional<at::Tensor>& mean,
                                     const c10::optional<at::Tensor>& invstd,
                                     const c10::optional<at::Tensor>& weight,
                                     const c10::optional<at::Tensor>& bias,
                                     const std::vector<int64_t>& res_map,
                                     const c10::optional<at::Tensor>& a2,
                                     const c10::optional<at::Tensor>& ebias,
                                     const c10::optional<at::Tensor>& scale,
                                     const c10::optional<at::Tensor>& shift, bool relu,
                                     const std::vector<int64_t>& a2_map) {
  check_bf16_2d(A, "A");
  check_bf16_2d(B, "B");
  const int64_t M = A.size(0), K1 = A.size(1), N = B.size(0);
  int64_t K = K1;
  const bool two = given(a2);
  XlOutMap a2m;
  if (two) {
    check_bf16_2d(*a2, "a2");
    int64_t rows = a2->size(0);
    if (!a2_map.empty()) {
      TORCH_CHECK(a2_map.size() == 5, "a2_map must be [stride, Ho, Wo, Hi, Wi]");
      a2m.s = (int)a2_map[0]; a2m.ho = (int)a2_map[1]; a2m.wo = (int)a2_map[2];
      a2m.hi = (int)a2_map[3]; a2m.wi = (int)a2_map[4];
      TORCH_CHECK(rows % ((int64_t)a2m.hi * a2m.wi) == 0, "a2_map does not match a2's rows");
      rows = rows / ((int64_t)a2m.hi * a2m.wi) * a2m.ho * a2m.wo;
    }
    TORCH_CHECK(rows == M && K1 % XBK == 0, "gemm_xl_conv: a2 must be [M (through a2_map), K2], K(A) % 64 == 0");
    K += a2->size(1);
  }
  TORCH_CHECK(B.size(1) == K && K % XBK == 0 && K >= XBK && N % 8 == 0, "gemm_xl_conv: bad shape");
  TORCH_CHECK(M > 0 && M < (1LL << 31), "gemm_xl_conv: M out of range");
  TORCH_CHECK(mode != "store", "gemm_xl_conv: use gemm_xl for a plain store");
  XlArgs a = xl_operands(A, A.stride(0), B, M, N, K);
  if (two) {
    a.A2 = bf16_ptr(*a2); a.lda2 = a2->stride(0); a.K1 = (int)K1;
    a.a2m = a2m;
  }
  XlConvEpi e;
  e.residual = residual;
  e.bn_x = bn_x; e.bn_y = bn_y;
  e.mean = mean; e.invstd = invstd; e.weight = weight; e.bias = bias;
  e.ebias = ebias;
  e.scale = scale; e.shift = shift; e.relu = relu;
  e.res_map = res_map;
  return xl_conv_run(a, A, mode, e);
}

// kh x kw convolution of an NHWC (channels-last) input as an implicit GEMM on
// the ping-pong kernel: C[N*Ho*Wo, Cout] = gather(x) @ wmat^T with wmat
// [Cout, kh*kw*Cin] (tap-major, channel-minor), padding taps read as zeros.
// mode "store" | "moments" | "add" | "bnbwd" (epilogues as gemm_xl_conv; the
// bnbwd / add operands are [N*Ho*Wo, Cout] row-major).  Returns (C, sums).
std::vector<at::Tensor> conv_xl(const at::Tensor& x, const at::Tensor& wmat, int64_t kh, int64_t kw,
                                int64_t stride, int64_t pad, int64_t ho, int64_t wo, const std::string& mode,
                                const c10::optional<at::Tensor>& residual,
                                const c10::optional<at::Tensor>& bn_x,
                                const c10::optional<at::Tensor>& bn_y,
                                const c10::optional<at::Tensor>& mean,
                                const c10::optional<at::Tensor>& invstd,
                                const c10::optional<at::Tensor>& weight,
                                const c10::optional<at::Tensor>& bias) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 4, "conv_xl: x must be 4-D bf16 GPU");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), "conv_xl: x must be channels_last");
  check_bf16_2d(wmat, "wmat");
  const int64_t nb = x.size(0), cin = x.size(1), hi = x.size(2), wi = x.size(3);
  TORCH_CHECK(cin % 64 == 0, "conv_xl: Cin must be a multiple of 64");
  TORCH_CHECK(wmat.size(1) == kh * kw * cin && wmat.size(0) % 8 == 0, "conv_xl: wmat must be [Cout, kh*kw*Cin]");
  TORCH_CHECK(ho > 0 && wo > 0 && stride >= 1 && pad >= 0 && (ho - 1) * stride - pad + kh - 1 < hi + pad &&
                  (wo - 1) * stride - pad + kw - 1 < wi + pad, "conv_xl: bad geometry");
  TORCH_CHECK(nb * ho * wo < (1LL << 31) && nb * hi * wi < (1LL << 31), "conv_xl: too many pixels");
  TORCH_CHECK(x.device() == wmat.device(), "conv_xl: device mismatch");
  XlArgs a = xl_operands(x, cin, wmat, nb * ho * wo, wmat.size(0), kh * kw * cin);
  a.cv = xl_conv_geom(cin, hi, wi, ho, wo, stride, pad, kw);
  XlConvEpi e;
  e.residual = residual;
  e.bn_x = bn_x; e.bn_y = bn_y;
  e.mean = mean; e.invstd = invstd; e.weight = weight; e.bias = bias;
  return xl_conv_run(a, x, mode, e);
}

// Data gradient of a 3x3 / stride-2 / pad-1 conv as four stride-phase
// implicit GEMMs on the ping-pong kernel (no zero-filled dx, no zero taps):
// dx[n, 2m + py, 2q + px, :] = sum over the taps (ky, kx) of phase (py, px) of
// dy[n, m + a(ky), q + a(kx), :] @ W[:, :, ky, kx], with a(1) = 0 for the even
// phase and a(2) = 0, a(0) = 1 for the odd one.  Each phase is a stride-1,
// pad-0 conv over dy with a 1x1 / 1x2 / 2x1 / 2x2 kernel (the gather's bounds
// check supplies the zero row / column past the edge), written through an
// output row map straight into its pixels of dx.  wph[2 py + px]:
// [Cin][taps_y][taps_x][Cout] flattened to [Cin, taps * Cout].
// dy: [N, Cout, Ho, Wo] channels_last; returns dx as [N*hi*wi, Cin].
at::Tensor conv_xl_dgrad_s2(const at::Tensor& dy, const std::vector<at::Tensor>& wph, int64_t hi, int64_t wi) {
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 && dy.dim() == 4 &&
                  dy.is_contiguous(at::MemoryFormat::ChannelsLast), "conv_xl_dgrad_s2: dy must be 4-D bf16 channels_last");
  TORCH_CHECK(wph.size() == 4, "conv_xl_dgrad_s2: four phase weight matrices");
  const int64_t nb = dy.size(0), cout = dy.size(1), ho = dy.size(2), wo = dy.size(3);
  TORCH_CHECK(cout % 64 == 0 && hi % 2 == 0 && wi % 2 == 0 && ho == hi / 2 && wo == wi / 2,
              "conv_xl_dgrad_s2: even input size, Ho = H / 2, Cout % 64 == 0");
  const int64_t cin = wph[0].size(0);
  TORCH_CHECK(cin % 256 == 0, "conv_xl_dgrad_s2: Cin must be a multiple of 256 (full 256-wide tiles)");
  TORCH_CHECK(nb * hi * wi < (1LL << 31), "conv_xl_dgrad_s2: too many pixels");
  auto dx = at::empty({nb * hi * wi, cin}, dy.options());
  hipStream_t s = at::hip::getCurrentHIPStream();
  for (int ph = 0; ph < 4; ++ph) {
    const int py = ph >> 1, px = ph & 1;
    const int ty = py ? 2 : 1, tx = px ? 2 : 1;
    const at::Tensor& w = wph[ph];
    check_bf16_2d(w, "wph");
    TORCH_CHECK(w.size(0) == cin && w.size(1) == ty * tx * cout && w.device() == dy.device(),
                "conv_xl_dgrad_s2: wph[", ph, "] must be [Cin, ", ty * tx, " * Cout]");
    XlArgs a = xl_operands(dy, cout, w, nb * ho * wo, cin, ty * tx * cout, dx);
    a.cv = xl_conv_geom(cout, ho, wo, ho, wo, 1, 0, tx);
    a.omap.s = 2; a.omap.ho = (int)ho; a.omap.wo = (int)wo; a.omap.hi = (int)hi; a.omap.wi = (int)wi;
    a.omap.oy = py; a.omap.ox = px;
    a.bm = pick_bm(a.M, a.N, a.K, XL_STORE);
    xl_launch(a, XL_STORE, 256, s);
  }
  DMP_HIP_CHECK(hipGetLastError());
  return dx;
}

void set_gemm_xl_trim_heavy(bool on) { g_xl_trim_heavy = on ? 1 : 0; }

int get_gemm_xl_pipe() { return g_xl_pipe; }
void set_gemm_xl_x2(int mode) {
  TORCH_CHECK(mode >= 0 && mode <= 2, "x2 mode: 0 off, 1 short K, 2 always");
  g_xl_x2 = mode;
}
int get_gemm_xl_x2() { return g_xl_x2; }
// The trace buffer is held here (not just its pointer) so a tensor freed by
// the caller can never receive timestamps; tracing cannot be switched on
// while a stream is being captured (the pointer would be baked into the graph).
at::Tensor g_xl_tbuf;
void set_gemm_xl_trace(const c10::optional<at::Tensor>& buf) {
  if (!buf || !buf->defined()) {
    g_xl_tdbg = nullptr;
    g_xl_tbuf = at::Tensor();
    return;
  }
  TORCH_CHECK(buf->is_cuda() && buf->scalar_type() == at::kLong && buf->is_contiguous(),
              "trace buffer: contiguous int64 GPU tensor of 8 entries per block");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  DMP_HIP_CHECK(hipStreamIsCapturing(at::hip::getCurrentHIPStream().stream(), &cs));
  TORCH_CHECK(cs == hipStreamCaptureStatusNone, "set_gemm_xl_trace: not while a stream is being captured");
  g_xl_tbuf = *buf;
  g_xl_tdbg = reinterpret_cast<unsigned long long*>(g_xl_tbuf.data_ptr());
}
void set_gemm_xl_bm(int bm) {
  TORCH_CHECK(bm == 0 || bm == -1 || (bm >= 192 && bm <= 256 && bm % 16 == 0),
              "bm: 0 (auto), -1 (always 256) or 192..256 in steps of 16");
  g_xl_bm = bm;
}
int get_gemm_xl_bm(int64_t M, int64_t N, int64_t K) { return pick_bm(M, N, K, XL_STORE); }

void set_gemm_xl_bn(int bn, int pipe, int group_m) {
  if (pipe < 0) pipe = kXlPipeDefault;
  TORCH_CHECK(group_m >= 0, "group_m must be >= 0 (0 = default)");
  g_xl_group_m = group_m;
  TORCH_CHECK(bn == 0 || bn == 128 || bn == 256, "bn must be 0 (auto), 128 or 256");
  TORCH_CHECK(pipe == 0 || pipe == 1 || pipe == 10 || pipe == 11,
              "pipe must be 0 / 1 (8-wave 256 x 128 / 256 x 256 ring kernels), 10 (8-wave ping-pong) or "
              "11 (4-wave, the default)");
  g_xl_bn_override = bn;
  g_xl_pipe = pipe;
}

}  // namespace dmp
