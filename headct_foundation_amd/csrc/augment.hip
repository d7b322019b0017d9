// Device side of the DINO multi-crop augmentation (DataAugmentationDINO3D, src/data/transforms.py:39-105).
//
//   hct_crop_resize_area : every view of a batch in ONE launch -- cast, zero-padded random box, area resize to F^3, axis
//                          flips, intensity shift.  The padded field of the reference is never materialised: a box is given
//                          in input-volume coordinates and whatever lies outside [0, S) reads as zero.
//   hct_adjust_contrast  : RandAdjustContrast in place: per-sample min / max over all channels (two launches, no
//                          floating-point atomics), then the gamma curve.
//
// and of the fine-tuning loader's device-resident pool (vit_transforms, src/data/transforms.py:258-320):
//
//   hct_gather_augment   : a batch out of the fp16 pool in ONE launch -- gather by slot index, axis flips, intensity shift,
//                          widening to fp32 (the arithmetic of hct_augment_volume; the gathered fp16 batch is never written).
//
// The first two are streaming kernels: one thread makes 4 consecutive fp32 outputs of the contiguous axis and stores them as 16 bytes,
// with ordinary (cacheable) stores because the patch gather of the backbone reads the crops next.
//
// Window sums go straight through L1 / L2, not through LDS-staged input tiles.  An output averages 1..4 voxels per axis
// (64 at most at the reference's sizes), neighbouring lanes read neighbouring windows of the same input rows, so the loads of
// a wave fall on a few cache lines, and a voxel is needed by at most two outputs per axis; staging a tile in LDS would add a
// barrier and a box-dependent tile shape to save re-reads that the 32 KB L1 already absorbs.  With the reference's geometry
// most outputs lie in the zero padding and issue no load at all, so the launch is bound by its stores.
#include "common.h"
#include "prof.h"

#include <limits.h>

#include <algorithm>

namespace hct {

// window of resized index i along an axis of n input voxels and F outputs (adaptive average pooling, = F.interpolate "area")
__device__ __forceinline__ void area_window(int i, int n, int F, int start, int& lo, int& hi) {
  lo = start + (i * n) / F;
  hi = start + ((i + 1) * n + F - 1) / F;
}

template <typename TIn>
__global__ void __launch_bounds__(256) crop_resize_area_kernel(const TIn* __restrict__ in, int B, int C, int S, float* __restrict__ out, int F,
                                                               const int32_t* __restrict__ boxes, const unsigned char* __restrict__ flip,
                                                               const float* __restrict__ shift, int per_vol4) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= per_vol4) return;
  const int f4 = F >> 2;
  const int k4 = t % f4;
  const int r = t / f4;
  const int j = r % F, i = r / F;
  const int vbc = blockIdx.y;  // (v * B + b) * C + c
  const int vb = vbc / C, c = vbc - vb * C, b = vb % B;
  const int32_t* bx = boxes + (int64_t)vb * 6;
  // the table lives on the device and cannot be checked by the host: a size outside the contract is clamped so that the index
  // arithmetic stays in range (loads are confined to [0, S) below whatever the box says)
  const int n0 = min(max(bx[3], 1), 65536), n1 = min(max(bx[4], 1), 65536), n2 = min(max(bx[5], 1), 65536);
  const int s0 = min(max(bx[0], -(1 << 24)), 1 << 24), s1 = min(max(bx[1], -(1 << 24)), 1 << 24), s2 = min(max(bx[2], -(1 << 24)), 1 << 24);
  const unsigned f = flip ? flip[vb] : 0u;
  const float sh = shift ? shift[vb] : 0.f;
  // a flip acts on the resized crop: output index i shows resized index F - 1 - i
  int x0, x1, y0, y1;
  area_window((f & 1u) ? F - 1 - i : i, n0, F, s0, x0, x1);
  area_window((f & 2u) ? F - 1 - j : j, n1, F, s1, y0, y1);
  const float nxy = (float)((x1 - x0) * (y1 - y0));
  x0 = max(x0, 0); x1 = min(x1, S);
  y0 = max(y0, 0); y1 = min(y1, S);
  int z0[4], z1[4];
  float cnt[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = k4 * 4 + q;
    area_window((f & 4u) ? F - 1 - k : k, n2, F, s2, z0[q], z1[q]);
    cnt[q] = nxy * (float)(z1[q] - z0[q]);  // voxels of the padding count: they are zeros of the field
    z0[q] = max(z0[q], 0); z1[q] = min(z1[q], S);
  }
  const TIn* vol = in + ((int64_t)b * C + c) * S * S * S;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  // fixed order: x, then y, then z ascending in input coordinates, whatever the flip
  for (int x = x0; x < x1; ++x)
    for (int y = y0; y < y1; ++y) {
      const TIn* row = vol + ((int64_t)x * S + y) * S;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        for (int z = z0[q]; z < z1[q]; ++z) acc[q] += to_f32(row[z]);
    }
  f32x4 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = acc[q] / cnt[q] + sh;
  Vec4<float>::store(out + (((int64_t)vbc * F + i) * F + j) * F + k4 * 4, o);
}

// ---- RandAdjustContrast ----------------------------------------------------------------------------------------------------
constexpr int kContrastMaxChunks = 256;
static int contrast_chunks(int64_t n) { return (int)std::min<int64_t>(kContrastMaxChunks, std::max<int64_t>(1, (n / 4 + 1023) / 1024)); }

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// min and max of a block's values -> every thread (256 threads = 4 waves)
__device__ __forceinline__ void block_minmax(float& mn, float& mx) {
  __shared__ float smn[4], smx[4];
  mn = wave_min(mn);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) {
    smn[threadIdx.x >> 6] = mn;
    smx[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
  mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
}

// partial [B][chunks][2]: min, max of chunk blockIdx.x of sample blockIdx.y
__global__ void __launch_bounds__(256) contrast_minmax_kernel(const float* __restrict__ x, int64_t n4, const unsigned char* __restrict__ apply,
                                                              float* __restrict__ partial) {
  const int b = blockIdx.y;
  if (!apply[b]) return;
  const float* xs = x + (int64_t)b * n4 * 4;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 v = Vec4<float>::load(xs + i * 4);
    mn = fminf(fminf(mn, fminf(v[0], v[1])), fminf(v[2], v[3]));
    mx = fmaxf(fmaxf(mx, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
  }
  block_minmax(mn, mx);
  if (threadIdx.x == 0) {
    float* p = partial + ((int64_t)b * gridDim.x + blockIdx.x) * 2;
    p[0] = mn;
    p[1] = mx;
  }
}

// ((x - mn) / (mx - mn + 1e-7)) ** gamma * (mx - mn) + mn, as MONAI's AdjustContrast writes it (fp32 throughout)
__global__ void __launch_bounds__(256) contrast_apply_kernel(float* __restrict__ x, int64_t n4, const float* __restrict__ gamma,
                                                             const unsigned char* __restrict__ apply, const float* __restrict__ partial) {
  const int b = blockIdx.y;
  if (!apply[b]) return;
  float mn = INFINITY, mx = -INFINITY;
  if (threadIdx.x < gridDim.x) {  // gridDim.x <= 256 chunks: one partial pair per thread
    const float* p = partial + ((int64_t)b * gridDim.x + threadIdx.x) * 2;
    mn = p[0];
    mx = p[1];
  }
  block_minmax(mn, mx);
  const float range = mx - mn, den = range + 1e-7f, g = gamma[b];
  float* xs = x + (int64_t)b * n4 * 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 v = Vec4<float>::load(xs + i * 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = powf((v[q] - mn) / den, g) * range + mn;
    Vec4<float>::store(xs + i * 4, v);
  }
}

// ---- gather + flips + shift out of the device-resident pool -------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

// V fp16 voxels of one row, widened; `rev`: in reversed order (the flip of the contiguous axis, done within the vector)
template <int V> struct PoolVec;
template <> struct PoolVec<8> {  // 16-byte load, two 16-byte stores
  static __device__ __forceinline__ void run(const f16* src, float* dst, bool rev, float sh, bool zero) {
    f16x8 h = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!zero) h = __builtin_nontemporal_load(reinterpret_cast<const f16x8*>(src));  // a pool item is read once per batch
    f32x4 a, b;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      a[q] = (float)(rev ? h[7 - q] : h[q]) + sh;
      b[q] = (float)(rev ? h[3 - q] : h[4 + q]) + sh;
    }
    Vec4<float>::store(dst, a);  // cacheable: the patch gather of the backbone reads the batch next
    Vec4<float>::store(dst + 4, b);
  }
};
template <> struct PoolVec<4> {  // S a multiple of 4 but not of 8: rows are only 8-byte aligned
  static __device__ __forceinline__ void run(const f16* src, float* dst, bool rev, float sh, bool zero) {
    f16x4 h = {0, 0, 0, 0};
    if (!zero) h = __builtin_nontemporal_load(reinterpret_cast<const f16x4*>(src));
    f32x4 a;
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = (float)(rev ? h[3 - q] : h[q]) + sh;
    Vec4<float>::store(dst, a);
  }
};

// grid (chunks of a volume, B * C); a thread makes V consecutive outputs of the contiguous axis per step.  Slot, flip and shift
// are uniform over the block (scalar loads).  A slot outside [0, n_slots) is never dereferenced: -1 is the all-zero placeholder
// by contract, anything else is clamped to it.
template <int V>
__global__ void __launch_bounds__(256) gather_augment_kernel(const f16* __restrict__ pool, const int32_t* __restrict__ slot,
                                                             float* __restrict__ out, int C, int S, int64_t n_slots,
                                                             const unsigned char* __restrict__ flip, const float* __restrict__ shift,
                                                             int per_vol) {
  const int bc = blockIdx.y;
  const int b = bc / C, c = bc - b * C;
  const int64_t sl = slot[b];
  const bool zero = sl < 0 || sl >= n_slots;
  const unsigned f = flip ? flip[b] : 0u;
  const float sh = shift ? shift[b] : 0.f;
  const int sv = S / V;
  const int64_t vol = (int64_t)S * S * S;
  const f16* src = pool + ((zero ? 0 : sl) * C + c) * vol;
  float* dst = out + (int64_t)bc * vol;
  const bool rev = (f & 4u) != 0;
  for (int u = blockIdx.x * 256 + threadIdx.x; u < per_vol; u += gridDim.x * 256) {
    const int kv = u % sv;
    const int r = u / sv;
    const int j = r % S, i = r / S;
    const int si = (f & 1u) ? S - 1 - i : i, sj = (f & 2u) ? S - 1 - j : j;
    const int sk = rev ? S - V - kv * V : kv * V;
    PoolVec<V>::run(src + ((int64_t)si * S + sj) * S + sk, dst + ((int64_t)i * S + j) * S + kv * V, rev, sh, zero);
  }
}

}  // namespace hct

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int hct_crop_resize_area(const void* in, int in_dtype, int B, int C, int S, float* out, int F, int n_views, const int32_t* boxes,
                         const unsigned char* flip, const float* shift, void* stream) {
  HCT_REQUIRE(in && out && boxes && (const void*)out != in, "hct_crop_resize_area: null argument");
  HCT_REQUIRE(B > 0 && C > 0 && S > 0 && S <= 4096 && n_views > 0 && F > 0 && F <= 4096 && F % 4 == 0,
              "hct_crop_resize_area: bad shape (B %d, C %d, S %d, F %d, views %d; F a multiple of 4; S at most 4096, F at most 2044)", B, C, S, F, n_views);
  HCT_REQUIRE(in_dtype == HCT_F32 || in_dtype == HCT_BF16 || in_dtype == HCT_F16, "hct_crop_resize_area: unsupported input dtype %d", in_dtype);
  HCT_REQUIRE((int64_t)n_views * B * C <= 65535, "hct_crop_resize_area: too many volumes in one launch (%lld)", (long long)n_views * B * C);
  // the kernel indexes a volume's F^3 / 4 threads, rounded up to whole blocks, in an int: F <= 2044
  const int64_t per_vol4_wide = (int64_t)F * F * (F / 4);
  HCT_REQUIRE(per_vol4_wide + 255 <= (int64_t)INT_MAX, "hct_crop_resize_area: F %d is too large (F * F * F / 4 + 255 must fit an int: F <= 2044)", F);
  const int per_vol4 = (int)per_vol4_wide;
  const dim3 grid((unsigned)((per_vol4 + 255) / 256), (unsigned)(n_views * B * C)), block(256);
  hipStream_t s = (hipStream_t)stream;
#define HCT_CRA(T) hipLaunchKernelGGL(hct::crop_resize_area_kernel<T>, grid, block, 0, s, (const T*)in, B, C, S, out, F, boxes, flip, shift, per_vol4)
  if (in_dtype == HCT_F32) HCT_CRA(float);
  else if (in_dtype == HCT_BF16) HCT_CRA(hct::bf16);
  else HCT_CRA(hct::f16);
#undef HCT_CRA
  HCT_CHECK_LAUNCH("hct_crop_resize_area");
  return 0;
}

size_t hct_adjust_contrast_workspace_bytes(int B, int64_t n) {
  if (B <= 0 || n <= 0) return 0;
  return (size_t)B * hct::contrast_chunks(n) * 2 * sizeof(float);
}

int hct_adjust_contrast(float* x, int B, int64_t n, const float* gamma, const unsigned char* apply, void* workspace, size_t workspace_bytes,
                        void* stream) {
  HCT_REQUIRE(x && gamma && apply && B > 0 && B <= 65535 && n > 0 && n % 4 == 0,
              "hct_adjust_contrast: bad arguments (values per sample must be a multiple of 4, at most 65535 samples)");
  HCT_REQUIRE(workspace && workspace_bytes >= hct_adjust_contrast_workspace_bytes(B, n), "hct_adjust_contrast: workspace too small");
  const dim3 grid((unsigned)hct::contrast_chunks(n), (unsigned)B), block(256);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(hct::contrast_minmax_kernel, grid, block, 0, s, (const float*)x, n / 4, apply, (float*)workspace);
  hipLaunchKernelGGL(hct::contrast_apply_kernel, grid, block, 0, s, x, n / 4, gamma, apply, (const float*)workspace);
  HCT_CHECK_LAUNCH("hct_adjust_contrast");
  return 0;
}

int hct_gather_augment(const void* pool, const int32_t* slot, float* out, int B, int C, int S, int64_t n_slots, const unsigned char* flip,
                       const float* shift, void* stream) {
  HCT_REQUIRE(pool && slot && out && B > 0 && C > 0 && S > 0 && S % 4 == 0 && S <= 1024 && n_slots > 0 && (const void*)out != pool,
              "hct_gather_augment: bad arguments (S must be a multiple of 4, at most 1024; the pool needs a slot)");
  HCT_REQUIRE((int64_t)B * C <= 65535, "hct_gather_augment: too many volumes in one launch (%lld)", (long long)B * C);
  HCT_REQUIRE((uintptr_t)out % 16 == 0 && (uintptr_t)pool % 8 == 0, "hct_gather_augment: out must be 16-byte, pool 8-byte aligned");
  const bool wide = S % 8 == 0 && (uintptr_t)pool % 16 == 0;
  const int per_vol = S * S * (S / (wide ? 8 : 4));
  // about 4096 blocks over the launch, each striding over its volume: enough to fill 256 CUs several times, few enough that
  // the per-block scalar set-up is paid a few dozen times per CU
  const int want = (4096 + B * C - 1) / (B * C);
  const dim3 grid((unsigned)std::max(1, std::min((per_vol + 255) / 256, want)), (unsigned)(B * C)), block(256);
  hipStream_t s = (hipStream_t)stream;
  const double voxels = (double)B * C * S * S * S;
  hct::ProfScope ps(hct::PROF_AUGMENT, voxels, s, 2.0 * voxels + 4.0 * voxels);
  if (wide) hipLaunchKernelGGL(hct::gather_augment_kernel<8>, grid, block, 0, s, (const hct::f16*)pool, slot, out, C, S, n_slots, flip, shift, per_vol);
  else hipLaunchKernelGGL(hct::gather_augment_kernel<4>, grid, block, 0, s, (const hct::f16*)pool, slot, out, C, S, n_slots, flip, shift, per_vol);
  HCT_CHECK_LAUNCH("hct_gather_augment");
  return 0;
}

}  // extern "C"
