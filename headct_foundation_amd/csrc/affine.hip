// Random 3-D affine augmentation of the fine-tuning loader (TRAIN.AFFINE_*; MONAI's RandAffine, which the reference leaves out).
//
//   hct_affine_augment : the whole train-time transform of a batch in ONE launch and one pass -- gather by slot index out of the fp16
//                        pool (or a stacked batch), per-sample 3 x 4 map from output to input coordinates, trilinear interpolation
//                        with zeros outside, intensity shift, widening to fp32.  No gathered, rotated or flipped intermediate is
//                        written.  A sample whose `fire` byte is 0 takes the flip / copy / shift arithmetic of hct_gather_augment.
//   hct_affine_labels  : the label volumes of a segmentation batch through the SAME table: uint8 out of a pool by slot index, the
//                        nearest voxel of the same coordinates (affine_map / affine_row / affine_coord below serve both kernels), a
//                        caller-chosen byte outside the volume.  A sample whose `fire` byte is 0 takes the copy of
//                        hct_gather_flip_labels.  Four byte loads and one 4-byte store per thread and trip.
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

// The map from an output voxel to its input coordinate, written ONCE for the image kernel and the label kernel, so that a scan and
// its mask cannot drift apart:  q_a = fma(A_a2, p_2, fma(A_a1, p_1, fma(A_a0, p_0, t_a + c))),  p = index - c,  c = (S - 1) / 2.
// affine_row is the part that is constant along the contiguous axis, affine_coord adds that axis.
struct AffineMap {
  float A[3][3], tc[3], cen;
};
__device__ __forceinline__ AffineMap affine_map(const float* __restrict__ m, int S) {
  AffineMap M;
  M.cen = 0.5f * (float)(S - 1);  // exact
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    M.A[a][0] = m[a * 4 + 0];
    M.A[a][1] = m[a * 4 + 1];
    M.A[a][2] = m[a * 4 + 2];
    M.tc[a] = m[a * 4 + 3] + M.cen;
  }
  return M;
}
__device__ __forceinline__ float affine_row(const AffineMap& M, int a, float p0, float p1) { return fmaf(M.A[a][1], p1, fmaf(M.A[a][0], p0, M.tc[a])); }
__device__ __forceinline__ float affine_coord(const AffineMap& M, int a, float row, float p2) { return fmaf(M.A[a][2], p2, row); }

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
  const AffineMap M = affine_map(mat + (int64_t)b * 12, S);
  const float cen = M.cen;
  const int SS = S * S;
  for (int u = blockIdx.x * 256 + threadIdx.x; u < per_vol4; u += gridDim.x * 256) {
    const int k4 = u % s4;
    const int r = u / s4;
    const int j = r % S, i = r / S;
    const float p0 = (float)i - cen, p1 = (float)j - cen;  // exact: half-integers below 2^11
    float row[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) row[a] = affine_row(M, a, p0, p1);
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
      const AxisTaps x = axis_taps(affine_coord(M, 0, row[0], p2), S);
      const AxisTaps y = axis_taps(affine_coord(M, 1, row[1], p2), S);
      const AxisTaps z = axis_taps(affine_coord(M, 2, row[2], p2), S);
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

// One axis of one label output: the nearest voxel n = floor(q + 0.5) (a tie q = n + 0.5 goes up) and whether q lies in the volume's
// cell range [-0.5, S - 0.5).  As in axis_taps the test is made on the floating-point value before any conversion, in a form a NaN
// fails.  floor(q) and the fraction q - floor(q) are exact where q >= 0, so the tie falls where the fp32 value of q puts it (q + 0.5f
// would round 0.5 - 2^-25 up to 1); for q in [-0.5, 0) the fraction is at least 0.5 however q + 1 rounds: n = 0.  n is in [0, S - 1]
// for every q that passes, and is clamped all the same: the address is formed whether or not the value is used.
__device__ __forceinline__ int nearest_voxel(float q, int S, bool& inside) {
  const bool ok = q >= -0.5f && q < (float)S - 0.5f;  // S <= 1024: S - 0.5 is exact
  const float qs = ok ? q : 0.0f;                     // never convert what failed the test
  const float fl = floorf(qs);
  const int n = (int)fl + ((qs - fl) >= 0.5f ? 1 : 0);
  inside = inside && ok;
  return min(max(n, 0), S - 1);
}

// grid (chunks of a volume, B).  pool [n_slots, S, S, S] uint8; a thread makes 4 consecutive labels of the contiguous axis and
// stores them as one word.  Label bytes are opaque: 255 travels like any other value.
__global__ void __launch_bounds__(256) affine_labels_kernel(const uint8_t* __restrict__ pool, const int32_t* __restrict__ slot, int64_t n_slots,
                                                            uint8_t* __restrict__ out, int S, const float* __restrict__ mat,
                                                            const unsigned char* __restrict__ fire, const unsigned char* __restrict__ flip,
                                                            uint32_t outside, int per_vol4) {
  const int b = blockIdx.y;
  const int64_t sl = slot[b];
  const bool none = sl < 0 || sl >= n_slots;  // the placeholder: nothing is read, every label is 255
  const int64_t vol = (int64_t)S * S * S;
  const uint8_t* src = pool + (none ? 0 : sl) * vol;  // every load below stays inside [src, src + vol)
  uint8_t* dst = out + (int64_t)b * vol;
  const int s4 = S >> 2;

  if (fire && !fire[b]) {
    // ---- the copy of gather_flip_labels_kernel: flip bits, one word in, one word out ----
    const unsigned f = flip ? flip[b] : 0u;
    const bool rev = (f & 4u) != 0;
    for (int u = blockIdx.x * 256 + threadIdx.x; u < per_vol4; u += gridDim.x * 256) {
      const int k4 = u % s4;
      const int r = u / s4;
      const int j = r % S, i = r / S;
      const int si = (f & 1u) ? S - 1 - i : i, sj = (f & 2u) ? S - 1 - j : j;
      const int sk = rev ? S - 4 - k4 * 4 : k4 * 4;
      uint32_t w = 0xffffffffu;
      if (!none) {
        w = *reinterpret_cast<const uint32_t*>(src + ((int64_t)si * S + sj) * S + sk);
        if (rev) w = __builtin_bswap32(w);
      }
      *reinterpret_cast<uint32_t*>(dst + ((int64_t)i * S + j) * S + k4 * 4) = w;
    }
    return;
  }

  // ---- affine path: the image kernel's coordinates, nearest voxel, `outside` where any axis leaves [-0.5, S - 0.5) ----
  const AffineMap M = affine_map(mat + (int64_t)b * 12, S);
  const int SS = S * S;
  for (int u = blockIdx.x * 256 + threadIdx.x; u < per_vol4; u += gridDim.x * 256) {
    const int k4 = u % s4;
    const int r = u / s4;
    const int j = r % S, i = r / S;
    uint32_t w = 0xffffffffu;
    if (!none) {  // uniform over the workgroup
      const float p0 = (float)i - M.cen, p1 = (float)j - M.cen;  // exact: half-integers below 2^11
      float row[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) row[a] = affine_row(M, a, p0, p1);
      unsigned off[4];  // offsets inside the volume, below S^3
      bool in[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float p2 = (float)(k4 * 4 + q) - M.cen;
        in[q] = true;
        const int n0 = nearest_voxel(affine_coord(M, 0, row[0], p2), S, in[q]);
        const int n1 = nearest_voxel(affine_coord(M, 1, row[1], p2), S, in[q]);
        const int n2 = nearest_voxel(affine_coord(M, 2, row[2], p2), S, in[q]);
        off[q] = (unsigned)(n0 * SS + n1 * S + n2);
      }
      // the four loads first, none behind a branch, from addresses inside the volume; the value is selected afterwards
      uint32_t v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = src[off[q]];
      w = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) w |= (in[q] ? v[q] : outside) << (8 * q);
    }
    *reinterpret_cast<uint32_t*>(dst + ((int64_t)i * S + j) * S + k4 * 4) = w;
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

int hct_affine_labels(const uint8_t* pool, const int32_t* slot, int64_t n_slots, uint8_t* out, int B, int S, const float* mat,
                      const unsigned char* fire, const unsigned char* flip, uint8_t outside, void* stream) {
  HCT_REQUIRE(pool && slot && out && B > 0 && B <= 65535 && S > 0 && S % 4 == 0 && S <= 1024 && n_slots > 0,
              "hct_affine_labels: bad arguments (S must be a multiple of 4, at most 1024; at most 65535 volumes; the pool needs a slot)");
  HCT_REQUIRE((const void*)out != pool, "hct_affine_labels: out must not be the pool");
  HCT_REQUIRE((uintptr_t)pool % 4 == 0 && (uintptr_t)out % 4 == 0, "hct_affine_labels: pool and out must be 4-byte aligned");
  HCT_REQUIRE(mat || !fire, "hct_affine_labels: fire without mat");
  if (!mat) return hct_gather_flip_labels(pool, slot, out, B, S, n_slots, flip, stream);  // the call IS the plain one
  const int per_vol4 = S * S * (S / 4);
  const int want = (4096 + B - 1) / B;  // the sizing of hct_gather_flip_labels
  const dim3 grid((unsigned)std::max(1, std::min((per_vol4 + 255) / 256, want)), (unsigned)B), block(256);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(hct::affine_labels_kernel, grid, block, 0, s, pool, slot, n_slots, out, S, mat, fire, flip, (uint32_t)outside, per_vol4);
  HCT_CHECK_LAUNCH("hct_affine_labels");
  return 0;
}

}  // extern "C"
