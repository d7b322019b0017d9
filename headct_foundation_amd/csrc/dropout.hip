// Dropout on the streaming sites (patch embedding, proj_drop, MLP drop1 / drop2; attentionblock.py:65, :97-98, patch_embedding.py:160,
// MONAI MLPBlock) and the keep mask itself.  Masks are counter-based (philox.h): element e of the row-major tensor a site acts on
// takes word e & 3 of Philox4x32-10(counter = (e >> 2, 0, site), key = seed); it is kept iff word >= floor(p 2^32) and kept values
// are scaled by 1 / (1 - p) in fp32.  One thread handles one group of four consecutive elements = one Philox call = one 16-byte
// (fp32) or 8-byte (bf16) access; the grid strides over the groups.
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
template <typename TI, typename TO>
__global__ void __launch_bounds__(256) dropout_apply_kernel(DropArgs a, const TI* x, TO* y, const float* residual,  // (y may be x, y2 may be x2: no restrict)
                                                            const TI* x2, TO* y2, int64_t batches, int64_t stride, int64_t off,
                                                            int64_t seg) {
  const int64_t gps = (seg + 3) >> 2;  // groups per segment
  const int64_t groups = batches * gps;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t b = g / gps, gi = g - b * gps;
    const int64_t e0 = b * stride + off + gi * 4;  // first element of the group
    const Philox4 w = drop_words_stream(a, (uint64_t)(e0 >> 2));
    if (gi * 4 + 4 <= seg) {
      f32x4 v = Vec4<TI>::load(x + e0);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] *= drop_mul(a, w.w[j]);
      if (residual) v += Vec4<float>::load(residual + e0);
      Vec4<TO>::store(y + e0, v);
      if (x2) {
        f32x4 v2 = Vec4<TI>::load(x2 + e0);
#pragma unroll
        for (int j = 0; j < 4; ++j) v2[j] *= drop_mul(a, w.w[j]);
        Vec4<TO>::store(y2 + e0, v2);
      }
    } else {  // ragged end of a segment
      for (int j = 0; gi * 4 + j < seg; ++j) {
        float v = to_f32(x[e0 + j]) * drop_mul(a, w.w[j]);
        if (residual) v += residual[e0 + j];
        y[e0 + j] = from_f32<TO>(v);
        if (x2) y2[e0 + j] = from_f32<TO>(to_f32(x2[e0 + j]) * drop_mul(a, w.w[j]));
      }
    }
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
  const int64_t groups = batches * ((seg + 3) / 4);
  if (groups == 0) return 0;
  const DropArgs a = make_drop_args(seed, site, p);
  hipStream_t s = (hipStream_t)stream;
  const int n_t = x2 ? 2 : 1;
  ProfScope ps(PROF_DROPOUT, (double)batches * seg * n_t, s,
               (double)batches * seg * (n_t * (dtype_size(x_dtype) + dtype_size(y_dtype)) + (residual ? 4.0 : 0.0)));
  const dim3 grid(grid_for(groups));
#define HCT_DROP_APPLY(TI_, TO_)                                                                                                             \
  hipLaunchKernelGGL((dropout_apply_kernel<TI_, TO_>), grid, dim3(256), 0, s, a, (const TI_*)x, (TO_*)y, residual, (const TI_*)x2, (TO_*)y2, \
                     batches, stride, off, seg)
  if (xf && yf) HCT_DROP_APPLY(float, float);
  else if (xf) HCT_DROP_APPLY(float, bf16);
  else if (yf) HCT_DROP_APPLY(bf16, float);
  else HCT_DROP_APPLY(bf16, bf16);
#undef HCT_DROP_APPLY
  HCT_CHECK_LAUNCH("hct_dropout_apply");
  return 0;
}

}  // extern "C"
