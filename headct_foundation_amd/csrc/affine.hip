// Random 3-D affine augmentation of the fine-tuning loader (TRAIN.AFFINE_*; MONAI's RandAffine, which the reference leaves out).
//
//   hct_affine_augment : the whole train-time transform of a batch in ONE launch and one pass -- gather by slot index out of the fp16
//                        pool (or a stacked batch), per-sample 3 x 4 map from output to input coordinates, trilinear interpolation
//                        with zeros outside, intensity shift, widening to fp32.  No gathered, rotated or flipped intermediate is
//                        written.  A sample whose `fire` byte is 0 takes the flip / copy / shift arithmetic of hct_gather_augment.
//
// A workgroup belongs to one sample (blockIdx.y = b): slot, fire, flip, shift and the twelve matrix entries are uniform over it
// (scalar loads), and the choice between the two paths never diverges within a wave.  A thread makes 4 consecutive outputs of the
// contiguous axis and stores them as 16 bytes, as the kernels of augment.hip do.  The coordinates, the eight weights and the tap
// offsets of its 4 outputs are computed once and kept in registers; the channels of the scan are a loop around the loads only.
//
// Taps go through L1 / L2 as per-lane loads; the launch is bound by their number, not by bytes (DESIGN.md has the measurements).
// What was tried, on [64, 3, 96^3] with every sample firing: eight 2-byte loads per output behind `if (tap inside)` branches, 2080 us;
// the same loads unconditional from clamped addresses with the value selected afterwards, so that a channel's loads are in flight
// together, 1592 us; the two taps of a row (adjacent along the contiguous axis) as ONE 4-byte load, 915 us -- this form.  Staging
// input rows in LDS was not tried.
#include "common.h"
#include "prof.h"

#include <algorithm>

namespace hct {

// One axis of one output: q is the input coordinate.  `ok` is decided on the floating-point value BEFORE any conversion to an
// integer, and in a form that a NaN fails; only then is the cell index taken, from a value known to lie in (-1, S).  f = floor(q)
// is in [-1, S - 1]; tap 0 is voxel f (valid where f >= 0), tap 1 is voxel f + 1 (valid where f + 1 < S), w1 = q - f, w0 = 1 - w1.
// i0 / i1 are the two voxel indices CLAMPED to [0, S - 1]: what a lane loads in place of a tap that is outside is a voxel of the
// same volume, and the loaded value is then replaced by zero (not multiplied by a zero weight: 0 * Inf would be NaN).
struct AxisTaps {
  int f, i0, i1;
  float w0, w1;
  bool v0, v1;
};
__device__ __forceinline__ AxisTaps axis_taps(float q, int S) {
  const bool ok = q > -1.0f && q < (float)S;
  const float qs = ok ? q : 0.0f;  // never convert what failed the test
  const float fl = floorf(qs);
  const int f = (int)fl;
  AxisTaps a;
  a.f = f;
  a.w1 = qs - fl;
  a.w0 = 1.0f - a.w1;
  a.v0 = ok && f >= 0;
  a.v1 = ok && f + 1 < S;
  a.i0 = min(max(f, 0), S - 1);
  a.i1 = min(max(f + 1, 0), S - 1);
  return a;
}

// Two voxels adjacent along the contiguous axis in ONE load (a 2-byte type: 4 bytes at 2-byte alignment; the compiler splits it
// where the target does not take unaligned loads).
template <typename T> struct Pair { T lo, hi; };
template <typename T> __device__ __forceinline__ Pair<T> load_pair(const T* p) {
  Pair<T> r;
  __builtin_memcpy(&r, p, sizeof(r));
  return r;
}

// grid (chunks of a volume, B).  in: the pool [n_slots, C, S, S, S] with slot != NULL, else the stacked batch [B, C, S, S, S].
template <typename TIn>
__global__ void __launch_bounds__(256) affine_augment_kernel(const TIn* __restrict__ in, const int32_t* __restrict__ slot, int64_t n_slots,
                                                             float* __restrict__ out, int C, int S, const float* __restrict__ mat,
                                                             const unsigned char* __restrict__ fire, const unsigned char* __restrict__ flip,
                                                             const float* __restrict__ shift, int per_vol4) {
  const int b = blockIdx.y;
  const int64_t sl = slot ? (int64_t)slot[b] : (int64_t)b;
  const bool zero = slot && (sl < 0 || sl >= n_slots);  // the placeholder volume: nothing is read for it
  const float sh = shift ? shift[b] : 0.f;
  const int64_t vol = (int64_t)S * S * S;
  const TIn* src = in + (zero ? 0 : sl) * C * vol;  // this sample's C volumes; every load below stays inside [src, src + C * vol)
  float* dst = out + (int64_t)b * C * vol;
  const int s4 = S >> 2;

  if (!mat || (fire && !fire[b])) {
    // ---- the arithmetic of hct_gather_augment / hct_augment_volume: flip bits, copy, shift ----
    const unsigned f = flip ? flip[b] : 0u;
    const bool rev = (f & 4u) != 0;
    for (int u = blockIdx.x * 256 + threadIdx.x; u < per_vol4; u += gridDim.x * 256) {
      const int k4 = u % s4;
      const int r = u / s4;
      const int j = r % S, i = r / S;
      const int si = (f & 1u) ? S - 1 - i : i, sj = (f & 2u) ? S - 1 - j : j;
      const int sk = rev ? S - 4 - k4 * 4 : k4 * 4;
      const int64_t so = ((int64_t)si * S + sj) * S + sk, dof = ((int64_t)i * S + j) * S + k4 * 4;
      for (int c = 0; c < C; ++c) {
        f32x4 h = {0.f, 0.f, 0.f, 0.f};
        if (!zero) h = Vec4<TIn>::load_nt(src + c * vol + so);  // an item is read once per batch
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = (rev ? h[3 - q] : h[q]) + sh;
        Vec4<float>::store(dst + c * vol + dof, o);  // cacheable: the patch gather of the backbone reads the batch next
      }
    }
    return;
  }

  // ---- affine path: q_a = fma(A_a2, p_2, fma(A_a1, p_1, fma(A_a0, p_0, t_a + c))),  p = index - c,  c = (S - 1) / 2 ----
  const float* m = mat + (int64_t)b * 12;
  const float cen = 0.5f * (float)(S - 1);  // exact
  float A[3][3], tc[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    A[a][0] = m[a * 4 + 0];
    A[a][1] = m[a * 4 + 1];
    A[a][2] = m[a * 4 + 2];
    tc[a] = m[a * 4 + 3] + cen;
  }
  const int SS = S * S;
  for (int u = blockIdx.x * 256 + threadIdx.x; u < per_vol4; u += gridDim.x * 256) {
    const int k4 = u % s4;
    const int r = u / s4;
    const int j = r % S, i = r / S;
    const float p0 = (float)i - cen, p1 = (float)j - cen;  // exact: half-integers below 2^11
    float row[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) row[a] = fmaf(A[a][1], p1, fmaf(A[a][0], p0, tc[a]));
    const int64_t dof = ((int64_t)i * S + j) * S + k4 * 4;
    if (zero) {  // the placeholder volume: nothing is read
      const float o1 = 0.f + sh;
      for (int c = 0; c < C; ++c) Vec4<float>::store(dst + c * vol + dof, f32x4{o1, o1, o1, o1});
      continue;
    }
    float w[4][8];
    unsigned oxy[4][4], oz[4];  // offsets inside a volume, oxy + oz + 1 < S^3: no tap's address can leave it
    unsigned valid[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float p2 = (float)(k4 * 4 + q) - cen;
      const AxisTaps x = axis_taps(fmaf(A[0][2], p2, row[0]), S);
      const AxisTaps y = axis_taps(fmaf(A[1][2], p2, row[1]), S);
      const AxisTaps z = axis_taps(fmaf(A[2][2], p2, row[2]), S);
      oxy[q][0] = (unsigned)(x.i0 * SS + y.i0 * S);
      oxy[q][1] = (unsigned)(x.i0 * SS + y.i1 * S);
      oxy[q][2] = (unsigned)(x.i1 * SS + y.i0 * S);
      oxy[q][3] = (unsigned)(x.i1 * SS + y.i1 * S);
      // the two taps along the contiguous axis are voxels zb, zb + 1 of one row, zb = clamp(f, 0, S - 2).  At the two borders the
      // pair is shifted against the taps: f = -1 has tap 1 in the pair's low half, f = S - 1 has tap 0 in its high half (the other
      // tap is outside and counts as zero)
      const int zb = min(max(z.f, 0), S - 2);
      oz[q] = (unsigned)zb;
      const float wxy[4] = {x.w0 * y.w0, x.w0 * y.w1, x.w1 * y.w0, x.w1 * y.w1};
      const bool vxy[4] = {x.v0 && y.v0, x.v0 && y.v1, x.v1 && y.v0, x.v1 && y.v1};
      unsigned bits = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        w[q][2 * t] = wxy[t] * z.w0;
        w[q][2 * t + 1] = wxy[t] * z.w1;
        bits |= (vxy[t] && z.v0 ? 1u : 0u) << (2 * t);
        bits |= (vxy[t] && z.v1 ? 1u : 0u) << (2 * t + 1);
      }
      valid[q] = bits | (z.f > zb ? 256u : 0u) | (z.f < zb ? 512u : 0u);
    }
    for (int c = 0; c < C; ++c) {
      const TIn* v = src + c * vol;
      // all 16 loads of a channel first, none behind a branch, so that they are in flight together
      Pair<TIn> pr[4][4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) pr[q][t] = load_pair(v + (oxy[q][t] + oz[q]));
      float tap[4][8];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float lo = to_f32(pr[q][t].lo), hi = to_f32(pr[q][t].hi);
          tap[q][2 * t] = (valid[q] & 256u) ? hi : lo;
          tap[q][2 * t + 1] = (valid[q] & 512u) ? lo : hi;
        }
      f32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float acc = 0.f;
        // taps in ascending (d0, d1, d2), d2 fastest; one outside the volume counts as the value zero
#pragma unroll
        for (int t = 0; t < 8; ++t) acc = fmaf(w[q][t], (valid[q] & (1u << t)) ? tap[q][t] : 0.f, acc);
        o[q] = acc + sh;
      }
      Vec4<float>::store(dst + c * vol + dof, o);
    }
  }
}

}  // namespace hct

extern "C" {

int hct_affine_augment(const void* in, int in_dtype, const int32_t* slot, int64_t n_slots, float* out, int B, int C, int S, const float* mat,
                       const unsigned char* fire, const unsigned char* flip, const float* shift, void* stream) {
  HCT_REQUIRE(in && out && (const void*)out != in, "hct_affine_augment: null argument (in and out are required and must differ)");
  HCT_REQUIRE(B > 0 && C > 0 && S > 0 && S % 4 == 0 && S <= 1024, "hct_affine_augment: bad shape (B %d, C %d, S %d; S a multiple of 4, at most 1024)",
              B, C, S);
  HCT_REQUIRE((int64_t)B * C <= 65535, "hct_affine_augment: too many volumes in one launch (%lld)", (long long)B * C);
  HCT_REQUIRE(in_dtype == HCT_F32 || in_dtype == HCT_BF16 || in_dtype == HCT_F16, "hct_affine_augment: unsupported input dtype %d", in_dtype);
  HCT_REQUIRE(!slot || (in_dtype == HCT_F16 && n_slots > 0), "hct_affine_augment: a pool is fp16 and needs a slot (dtype %d, %lld slots)", in_dtype,
              (long long)n_slots);
  HCT_REQUIRE(mat || !fire, "hct_affine_augment: fire without mat");
  HCT_REQUIRE((uintptr_t)out % 16 == 0 && (uintptr_t)in % (in_dtype == HCT_F32 ? 16 : 8) == 0,
              "hct_affine_augment: out (and an fp32 in) must be 16-byte aligned, a 2-byte in 8-byte aligned");
  if (!mat)  // the call IS the plain one
    return slot ? hct_gather_augment(in, slot, out, B, C, S, n_slots, flip, shift, stream) : hct_augment_volume(in, in_dtype, out, B, C, S, flip, shift, stream);
  const int per_vol4 = S * S * (S / 4);
  // about 4096 blocks over the launch, each striding over its sample (the sizing of hct_gather_augment)
  const int want = (4096 + B - 1) / B;
  const dim3 grid((unsigned)std::max(1, std::min((per_vol4 + 255) / 256, want)), (unsigned)B), block(256);
  hipStream_t s = (hipStream_t)stream;
  const double voxels = (double)B * C * S * S * S;
  hct::ProfScope ps(hct::PROF_AUGMENT, voxels, s, 2.0 * voxels + 4.0 * voxels);
#define HCT_AFF(T) hipLaunchKernelGGL(hct::affine_augment_kernel<T>, grid, block, 0, s, (const T*)in, slot, n_slots, out, C, S, mat, fire, flip, shift, per_vol4)
  if (in_dtype == HCT_F32) HCT_AFF(float);
  else if (in_dtype == HCT_BF16) HCT_AFF(hct::bf16);
  else HCT_AFF(hct::f16);
#undef HCT_AFF
  HCT_CHECK_LAUNCH("hct_affine_augment");
  return 0;
}

}  // extern "C"
