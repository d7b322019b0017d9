// Mixup, CutMix and label smoothing of the fine-tuning recipe (additions of this build; the reference has neither).
//
//   hct_mix_volumes : mixes every sample of a [B, C, S, S, S] fp32 batch with its partner B - 1 - b IN PLACE, one launch.  Both
//                     outputs of a pair need both inputs from before the call, so the thread that owns a voxel of the pair loads
//                     both members, computes both and stores both, and no other thread touches that voxel of either sample: one
//                     read and one write per voxel (8 bytes), against the flip copy + mul_ + add_ of a torch composition (28).
//                     A member with a box (CutMix) takes bit copies of its partner inside the box and keeps the rest; rows and
//                     vectors that no box of the pair reaches are neither loaded nor stored.
//   hct_mix_xent    : cross-entropy against the soft target the mix implies (two smoothed one-hot rows weighted by lam), which is
//                     never materialised; loss and logit gradient in the form of hct_softmax_xent.
#include "common.h"

#include <algorithm>

namespace hct {

// what one member of a pair does with its voxels; uniform over the block
struct MixSide {
  float lam, rest;  // rest = 1 - lam
  int lo0, hi0, lo1, hi1, lo2, hi2;
  bool boxed;       // CutMix: copy the partner inside the box, lam unused
  bool still;       // no voxel of this member changes (mixing with lam == 1)
};

// The table lives on the device and cannot be refused by the host: every bound is clamped to [0, S], and a box that is empty on
// any axis after that is no box (the member then mixes with its lam).
__device__ __forceinline__ MixSide mix_side(const float* __restrict__ lam, const int32_t* __restrict__ box, int b, int S) {
  MixSide m;
  m.lam = lam[b];
  m.rest = 1.0f - m.lam;
  m.lo0 = m.hi0 = m.lo1 = m.hi1 = m.lo2 = m.hi2 = 0;
  m.boxed = false;
  if (box) {
    const int32_t* bx = box + (int64_t)b * 6;
    m.lo0 = min(max(bx[0], 0), S); m.hi0 = min(max(bx[1], 0), S);
    m.lo1 = min(max(bx[2], 0), S); m.hi1 = min(max(bx[3], 0), S);
    m.lo2 = min(max(bx[4], 0), S); m.hi2 = min(max(bx[5], 0), S);
    m.boxed = m.lo0 < m.hi0 && m.lo1 < m.hi1 && m.lo2 < m.hi2;
  }
  m.still = !m.boxed && m.lam == 1.0f;
  return m;
}

// does the member change anything in the 4 voxels [k, k + 4) of row (i, j)
__device__ __forceinline__ bool mix_touches(const MixSide& m, int i, int j, int k) {
  if (!m.boxed) return !m.still;
  return i >= m.lo0 && i < m.hi0 && j >= m.lo1 && j < m.hi1 && k < m.hi2 && k + 4 > m.lo2;
}

// new values of a member: `own` its voxels, `other` its partner's, both from before the call
__device__ __forceinline__ f32x4 mix_vec(const MixSide& m, f32x4 own, f32x4 other, int k) {
  f32x4 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (m.boxed) o[q] = (k + q >= m.lo2 && k + q < m.hi2) ? other[q] : own[q];  // a float4 may straddle a face of the box
    else o[q] = fmaf(m.lam, own[q], m.rest * other[q]);
  }
  return o;
}

// grid (chunks of a volume, ceil(B / 2) * C pairs of volumes); a thread owns 4 consecutive voxels of the contiguous axis of BOTH
// members of its pair per step.  lam and box of both members are uniform over the block (scalar loads), as slot, flip and shift are
// in gather_augment_kernel.
__global__ void __launch_bounds__(256) mix_volumes_kernel(float* __restrict__ x, int B, int C, int S, const float* __restrict__ lam,
                                                          const int32_t* __restrict__ box, int per_vol4) {
  const int qc = blockIdx.y;
  const int b = qc / C, c = qc - b * C;
  const int p = B - 1 - b;
  if (p == b) return;  // the middle sample of an odd batch is its own partner
  const MixSide mb = mix_side(lam, box, b, S), mp = mix_side(lam, box, p, S);
  if (mb.still && mp.still) return;
  const int64_t vol = (int64_t)S * S * S;
  float* xb = x + ((int64_t)b * C + c) * vol;
  float* xp = x + ((int64_t)p * C + c) * vol;
  const int s4 = S >> 2;
  for (int u = blockIdx.x * 256 + threadIdx.x; u < per_vol4; u += gridDim.x * 256) {
    const int k = (u % s4) * 4;
    const int r = u / s4;
    const int j = r % S, i = r / S;
    const bool tb = mix_touches(mb, i, j, k), tp = mix_touches(mp, i, j, k);
    if (!tb && !tp) continue;
    const int64_t off = ((int64_t)i * S + j) * S + k;
    const f32x4 a = Vec4<float>::load(xb + off), d = Vec4<float>::load(xp + off);
    // cacheable stores: the patch gather of the backbone reads the batch next
    if (tb) Vec4<float>::store(xb + off, mix_vec(mb, a, d, k));
    if (tp) Vec4<float>::store(xp + off, mix_vec(mp, d, a, k));
  }
}

// Soft-target cross-entropy, one workgroup, rows folded in a fixed order (the form of softmax_xent_kernel).  With
// s(y)[c] = on [c == y] + off, on = 1 - smoothing, off = smoothing / Cn:  t[c] = lam s(y_b)[c] + (1 - lam) s(y_p)[c], p = B - 1 - b.
// A row's loss is sum_c t[c] (log z - (l[c] - m)) with m the row maximum and z = sum exp(l - m): the difference l[c] - m is taken
// first, so a row of large equal logits loses nothing to the rounding of log z + m.
__global__ void __launch_bounds__(256) mix_xent_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                       const float* __restrict__ lam, float smoothing, int B, int Cn,
                                                       const float* __restrict__ dloss, float* __restrict__ loss,
                                                       float* __restrict__ dlogits) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  // the gradient is ((softmax - t) / B) * g, the caller's scale last: a loss scaled by k then gives fl(k * gradient), bit for bit
  const float g = dloss ? dloss[0] : 1.0f, fB = (float)B;
  const float on = 1.0f - smoothing, off = smoothing / (float)Cn;
  float acc = 0.f;
  for (int b = tid; b < B; b += 256) {
    const float* l = logits + (size_t)b * Cn;
    const int64_t yb = target[b], yp = target[B - 1 - b];  // compared with c only, never an index
    const float wb = lam ? lam[b] : 1.0f, wp = 1.0f - wb;
    float m = -INFINITY;
    for (int c = 0; c < Cn; ++c) m = fmaxf(m, l[c]);
    float z = 0.f;
    for (int c = 0; c < Cn; ++c) z += expf(l[c] - m);
    const float lz = logf(z), iz = 1.0f / z;
    float row = 0.f;
    for (int c = 0; c < Cn; ++c) {
      const float sb = ((int64_t)c == yb ? on : 0.0f) + off;
      const float t = lam ? wb * sb + wp * (((int64_t)c == yp ? on : 0.0f) + off) : sb;
      const float d = l[c] - m;
      row += t * (lz - d);
      if (dlogits) dlogits[(size_t)b * Cn + c] = (expf(d) * iz - t) / fB * g;
    }
    acc += row;
  }
  red[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0 && loss) loss[0] = red[0] / (float)B;
}

}  // namespace hct

extern "C" {

int hct_mix_volumes(float* x, int B, int C, int S, const float* lam, const int32_t* box, void* stream) {
  HCT_REQUIRE(x && lam, "hct_mix_volumes: null argument (x and lam are required; box may be NULL)");
  HCT_REQUIRE(B > 0 && C > 0 && S > 0 && S % 4 == 0 && S <= 1024, "hct_mix_volumes: bad shape (B %d, C %d, S %d; S a multiple of 4, at most 1024)",
              B, C, S);
  HCT_REQUIRE((int64_t)B * C <= 65535, "hct_mix_volumes: too many volumes in one launch (%lld)", (long long)B * C);
  HCT_REQUIRE((uintptr_t)x % 16 == 0, "hct_mix_volumes: x must be 16-byte aligned");
  const int pairs = (B + 1) / 2 * C;
  const int per_vol4 = S * S * (S / 4);
  // about 4096 blocks over the launch, each striding over its pair of volumes (the sizing of hct_gather_augment)
  const int want = (4096 + pairs - 1) / pairs;
  const dim3 grid((unsigned)std::max(1, std::min((per_vol4 + 255) / 256, want)), (unsigned)pairs), block(256);
  hipLaunchKernelGGL(hct::mix_volumes_kernel, grid, block, 0, (hipStream_t)stream, x, B, C, S, lam, box, per_vol4);
  HCT_CHECK_LAUNCH("hct_mix_volumes");
  return 0;
}

int hct_mix_xent(const float* logits, const int64_t* target, const float* lam, float smoothing, int B, int n_classes, const float* dloss,
                 float* loss, float* dlogits, void* stream) {
  HCT_REQUIRE(logits && target && B > 0 && n_classes > 0 && (loss || dlogits),
              "hct_mix_xent: bad arguments (logits [B, n_classes] and target [B] with B, n_classes >= 1, and at least one of loss, dlogits)");
  HCT_REQUIRE(smoothing >= 0.0f && smoothing < 1.0f, "hct_mix_xent: smoothing must lie in [0, 1), got %g", (double)smoothing);
  hipLaunchKernelGGL(hct::mix_xent_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, target, lam, smoothing, B, n_classes, dloss,
                     loss, dlogits);
  HCT_CHECK_LAUNCH("hct_mix_xent");
  return 0;
}

}  // extern "C"
