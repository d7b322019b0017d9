// Dropout on the streaming sites (patch embedding, proj_drop, MLP drop1 / drop2; attentionblock.py:65, :97-98, patch_embedding.py:160,
// MONAI MLPBlock) and the keep mask itself.  Masks are counter-based (philox.h): element e of the row-major tensor a site acts on
// takes word e & 3 of Philox4x32-10(counter = (e >> 2, 0, site), key = seed); it is kept iff word >= floor(p 2^32) and kept values
// are scaled by 1 / (1 - p) in fp32.  One thread handles one group of four consecutive elements = one Philox call = one 16-byte
// (fp32) or 8-byte (bf16) access; the grid strides over the groups.
// Stochastic depth (drop path) rides on the proj_drop / drop2 sites: sample b of a branch takes word b & 3 of
// Philox4x32-10(counter = (b >> 2, 0, 1, site), key = seed), is kept iff word >= floor(q 2^32) and then scaled by 1 / (1 - q) in fp32
// (hct_drop_path_scales writes these multipliers as a table; hct_residual_drop_apply is the streaming pass with a table row).
#include "common.h"
#include "philox.h"
#include "prof.h"

#include <algorithm>

namespace hct {
namespace {

constexpr int kDropBlocks = 1024;  // grid cap: four workgroups of four waves per CU

// keep mask of a streaming tensor of n elements
__global__ void __launch_bounds__(256) dropout_mask_stream_kernel(DropArgs a, int64_t n, unsigned char* __restrict__ out) {
  const int64_t groups = (n + 3) >> 2;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const Philox4 w = drop_words_stream(a, (uint64_t)g);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (g * 4 + j < n) out[g * 4 + j] = w.w[j] >= a.thresh ? 1 : 0;
  }
}

// keep mask of the attention probabilities [BH, N, N]
__global__ void __launch_bounds__(256) dropout_mask_attn_kernel(DropArgs a, int BH, int N, unsigned char* __restrict__ out) {
  const int kg = (N + 3) >> 2;
  const int64_t groups = (int64_t)BH * N * kg;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int k4 = (int)(g % kg);
    const int64_t row = g / kg;  // bh * N + q
    const int q = (int)(row % N), bh = (int)(row / N);
    const Philox4 w = drop_words_attn(a, (uint32_t)k4, (uint32_t)q, (uint32_t)bh);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (k4 * 4 + j < N) out[row * N + k4 * 4 + j] = w.w[j] >= a.thresh ? 1 : 0;
  }
}

// y = x * Z (+ residual), and y2 = x2 * Z with the same mask, on `batches` segments of `seg` elements that start at element
// b * stride + off of the tensor the site acts on (the element index of the mask is the index in that whole tensor).
// Segment starts are multiples of 4 elements, so a group never straddles a Philox call.
// kPath (hct_residual_drop_apply): segment b is sample b and every multiplier of it is multiplied by scales[b], the sample's drop-path
// multiplier (0 or 1 / (1 - q)): c = fl(z * s_b), y = fl(fl(x * c) + residual).  kElems = false is rate p = 0: z = 1, no Philox call.
template <typename TI, typename TO, bool kElems, bool kPath>
__global__ void __launch_bounds__(256) dropout_apply_kernel(DropArgs a, const TI* x, TO* y, const float* residual,  // (y may be x, y2 may be x2: no restrict)
                                                            const TI* x2, TO* y2, int64_t batches, int64_t stride, int64_t off,
                                                            int64_t seg, const float* __restrict__ scales) {
  const int64_t gps = (seg + 3) >> 2;  // groups per segment
  const int64_t groups = batches * gps;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t b = g / gps, gi = g - b * gps;
    const int64_t e0 = b * stride + off + gi * 4;  // first element of the group
    float c[4];                                    // the four multipliers
    if constexpr (kElems) {
      const Philox4 w = drop_words_stream(a, (uint64_t)(e0 >> 2));
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = drop_mul(a, w.w[j]);
    }
    if constexpr (kPath) {
      const float sb = scales[b];
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = kElems ? c[j] * sb : sb;
    }
    if (gi * 4 + 4 <= seg) {
      f32x4 v = Vec4<TI>::load(x + e0);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] *= c[j];
      if (residual) v += Vec4<float>::load(residual + e0);
      Vec4<TO>::store(y + e0, v);
      if (x2) {
        f32x4 v2 = Vec4<TI>::load(x2 + e0);
#pragma unroll
        for (int j = 0; j < 4; ++j) v2[j] *= c[j];
        Vec4<TO>::store(y2 + e0, v2);
      }
    } else {  // ragged end of a segment
      for (int j = 0; gi * 4 + j < seg; ++j) {
        float v = to_f32(x[e0 + j]) * c[j];
        if (residual) v += residual[e0 + j];
        y[e0 + j] = from_f32<TO>(v);
        if (x2) y2[e0 + j] = from_f32<TO>(to_f32(x2[e0 + j]) * c[j]);
      }
    }
  }
}

// Drop-path multipliers (DESIGN.md "Dropout", stochastic depth): row r of out [n_sites, B] holds, for sample b, 1 / (1 - q_r) where word
// b & 3 of Philox4x32-10(counter = (b >> 2, 0, 1, site_r), key = seed) is >= floor(q_r 2^32), else 0.  The third counter word is 1 where
// the element masks have 0, so the two families never share a counter.  A row of rate 0 is all 1.0 and draws nothing.
constexpr int kPathRows = 128;  // rows of one launch (two per block: 64 blocks)
struct PathRows {
  uint32_t site[kPathRows], thresh[kPathRows];
  float scale[kPathRows];
};
__global__ void __launch_bounds__(256) drop_path_scales_kernel(PathRows t, uint32_t seed_lo, uint32_t seed_hi, int rows, int B, float* __restrict__ out) {
  const int gpr = (B + 3) >> 2;  // groups of four samples per row
  const int64_t groups = (int64_t)rows * gpr;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int r = (int)(g / gpr), gi = (int)(g - (int64_t)r * gpr);
    float m[4] = {1.f, 1.f, 1.f, 1.f};
    if (t.thresh[r] != 0u) {
      const Philox4 w = philox4x32_10((uint32_t)gi, 0u, 1u, t.site[r], seed_lo, seed_hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) m[j] = w.w[j] >= t.thresh[r] ? t.scale[r] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (gi * 4 + j < B) out[(int64_t)r * B + gi * 4 + j] = m[j];
  }
}

int grid_for(int64_t groups) { return (int)std::min<int64_t>(kDropBlocks, (groups + 255) / 256); }

}  // namespace

int check_drop_rate(const char* who, float p) {
  if (!(p >= 0.f) || !(p < 1.f)) {
    set_error("%s: the dropout rate must satisfy 0 <= p < 1 (p = 1 drops everything and has no finite scale), got %g", who, (double)p);
    return HCT_E_BADARG;
  }
  return 0;
}

// launch of the streaming pass for the checked arguments of hct_dropout_apply / hct_residual_drop_apply (scales: the latter's table row)
static int launch_apply(const char* who, const void* x, int x_dtype, void* y, int y_dtype, const float* residual, const void* x2, void* y2, int64_t batches,
                 int64_t stride, int64_t off, int64_t seg, uint64_t seed, int site, float p, const float* scales, hipStream_t s) {
  const bool xf = x_dtype == HCT_F32, yf = y_dtype == HCT_F32;
  const int64_t groups = batches * ((seg + 3) / 4);
  if (groups == 0) return 0;
  const DropArgs a = make_drop_args(seed, site, p);
  const int n_t = x2 ? 2 : 1;
  ProfScope ps(PROF_DROPOUT, (double)batches * seg * n_t, s,
               (double)batches * seg * (n_t * (dtype_size(x_dtype) + dtype_size(y_dtype)) + (residual ? 4.0 : 0.0)));
  const dim3 grid(grid_for(groups));
#define HCT_DROP_APPLY_(TI_, TO_, E_, P_)                                                                                                 \
  hipLaunchKernelGGL((dropout_apply_kernel<TI_, TO_, E_, P_>), grid, dim3(256), 0, s, a, (const TI_*)x, (TO_*)y, residual, (const TI_*)x2, \
                     (TO_*)y2, batches, stride, off, seg, scales)
#define HCT_DROP_APPLY(TI_, TO_)                                      \
  do {                                                                \
    if (!scales) HCT_DROP_APPLY_(TI_, TO_, true, false);              \
    else if (a.thresh != 0u) HCT_DROP_APPLY_(TI_, TO_, true, true);   \
    else HCT_DROP_APPLY_(TI_, TO_, false, true);                      \
  } while (0)
  if (xf && yf) HCT_DROP_APPLY(float, float);
  else if (xf) HCT_DROP_APPLY(float, bf16);
  else if (yf) HCT_DROP_APPLY(bf16, float);
  else HCT_DROP_APPLY(bf16, bf16);
#undef HCT_DROP_APPLY
#undef HCT_DROP_APPLY_
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return check_hip(e, who);
  return 0;
}

}  // namespace hct

using namespace hct;

extern "C" {

int hct_dropout_mask(uint64_t seed, int site, int kind, int64_t n, int BH, int N, float p, unsigned char* out, void* stream) {
  if (int rc = check_drop_rate("hct_dropout_mask", p)) return rc;
  HCT_REQUIRE(out && site >= 0 && (kind == 0 || kind == 1), "hct_dropout_mask: null output, negative site or kind not 0 (streaming) / 1 (attention)");
  const DropArgs a = make_drop_args(seed, site, p);
  if (kind == 0) {
    HCT_REQUIRE(n >= 0, "hct_dropout_mask: n < 0");
    if (n == 0) return 0;
    hipLaunchKernelGGL(dropout_mask_stream_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, n, out);
  } else {
    HCT_REQUIRE(BH > 0 && N > 0, "hct_dropout_mask: bad attention shape BH=%d N=%d", BH, N);
    hipLaunchKernelGGL(dropout_mask_attn_kernel, dim3(grid_for((int64_t)BH * N * ((N + 3) / 4))), dim3(256), 0, (hipStream_t)stream, a, BH, N, out);
  }
  HCT_CHECK_LAUNCH("hct_dropout_mask");
  return 0;
}

int hct_dropout_apply(const void* x, int x_dtype, void* y, int y_dtype, const float* residual, const void* x2, void* y2, int64_t batches,
                      int64_t stride, int64_t off, int64_t seg, uint64_t seed, int site, float p, void* stream) {
  if (int rc = check_drop_rate("hct_dropout_apply", p)) return rc;
  HCT_REQUIRE(x && y && site >= 0 && batches >= 0 && seg >= 0 && off >= 0, "hct_dropout_apply: null tensor, negative site or negative extent");
  HCT_REQUIRE((x2 == nullptr) == (y2 == nullptr), "hct_dropout_apply: x2 and y2 come together");
  HCT_REQUIRE(off % 4 == 0 && (batches <= 1 || (stride % 4 == 0 && off + seg <= stride)),
              "hct_dropout_apply: segments start on multiples of 4 elements and lie inside their stride (stride %lld off %lld seg %lld)", (long long)stride,
              (long long)off, (long long)seg);
  HCT_REQUIRE(!residual || y_dtype == HCT_F32, "hct_dropout_apply: the residual form writes fp32");
  const bool xf = x_dtype == HCT_F32, yf = y_dtype == HCT_F32;
  HCT_REQUIRE((xf || x_dtype == HCT_BF16) && (yf || y_dtype == HCT_BF16), "hct_dropout_apply: tensors are fp32 or bf16");
  return launch_apply("hct_dropout_apply", x, x_dtype, y, y_dtype, residual, x2, y2, batches, stride, off, seg, seed, site, p, nullptr, (hipStream_t)stream);
}

int hct_drop_path_scales(uint64_t seed, const int* sites, const float* rates, int n_sites, int B, float* out, void* stream) {
  HCT_REQUIRE(sites && rates && out && n_sites >= 0 && B > 0, "hct_drop_path_scales: null argument, n_sites < 0 or B <= 0");
  for (int i = 0; i < n_sites; ++i) {
    if (int rc = check_drop_rate("hct_drop_path_scales", rates[i])) return rc;
    HCT_REQUIRE(sites[i] >= 0, "hct_drop_path_scales: negative site %d", sites[i]);
  }
  for (int r0 = 0; r0 < n_sites; r0 += kPathRows) {  // (one launch up to 128 rows = 64 blocks)
    const int rows = std::min(kPathRows, n_sites - r0);
    PathRows t;
    for (int i = 0; i < rows; ++i) {
      const DropArgs a = make_drop_args(seed, sites[r0 + i], rates[r0 + i]);
      t.site[i] = a.site; t.thresh[i] = a.thresh; t.scale[i] = a.scale;
    }
    for (int i = rows; i < kPathRows; ++i) { t.site[i] = 0; t.thresh[i] = 0; t.scale[i] = 1.f; }
    hipLaunchKernelGGL(drop_path_scales_kernel, dim3(grid_for((int64_t)rows * ((B + 3) / 4))), dim3(256), 0, (hipStream_t)stream, t, (uint32_t)seed,
                       (uint32_t)(seed >> 32), rows, B, out + (int64_t)r0 * B);
    HCT_CHECK_LAUNCH("hct_drop_path_scales");
  }
  return 0;
}

int hct_residual_drop_apply(const void* x, int x_dtype, void* y, int y_dtype, const float* residual, int64_t B, int64_t seg, const float* scales,
                            uint64_t seed, int site, float p, void* stream) {
  if (int rc = check_drop_rate("hct_residual_drop_apply", p)) return rc;
  HCT_REQUIRE(x && y && scales && site >= 0 && B >= 0 && seg >= 0, "hct_residual_drop_apply: null tensor, negative site or negative extent");
  HCT_REQUIRE(B <= 1 || seg % 4 == 0, "hct_residual_drop_apply: with more than one sample the segment length is a multiple of 4 (seg %lld)", (long long)seg);
  HCT_REQUIRE(!residual || y_dtype == HCT_F32, "hct_residual_drop_apply: the residual form writes fp32");
  HCT_REQUIRE((x_dtype == HCT_F32 || x_dtype == HCT_BF16) && (y_dtype == HCT_F32 || y_dtype == HCT_BF16), "hct_residual_drop_apply: tensors are fp32 or bf16");
  return launch_apply("hct_residual_drop_apply", x, x_dtype, y, y_dtype, residual, nullptr, nullptr, B, seg, 0, seg, seed, site, p, scales, (hipStream_t)stream);
}

}  // extern "C"
