// Per-parameter gradient clip + AdamW / Lion / SGD / Lamb over one flat fp32 buffer (HBM-bound; one pass each, Lamb two + a fold).
//   reference: src/utils/misc.py:374-383 (per-tensor clip), src/utils/optimizers.py:354-360 (torch AdamW), :267-279 (Lion),
//   :347-353 (torch SGD), :154-172 (lamb_kernel).
// The flat buffer is cut into 1024-element units (one float4 per thread of a 256-thread block); every
// segment (= parameter tensor) starts on a unit boundary, so a unit belongs to exactly one segment.
#include "common.h"

namespace hct {

constexpr int kUnit = 1024;

__device__ __forceinline__ float block_sum_256(float v, float* s_tmp) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_tmp[0] + s_tmp[1]) + (s_tmp[2] + s_tmp[3]);
}

__global__ void __launch_bounds__(256) sumsq_units_kernel(const float* __restrict__ g, int64_t total,
                                                          float* __restrict__ unit_sumsq) {
  __shared__ float s_tmp[4];
  const int64_t i = (int64_t)blockIdx.x * kUnit + threadIdx.x * 4;
  float s = 0.f;
  if (i < total) {
    const f32x4 v = Vec4<float>::load(g + i);
    s = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  s = block_sum_256(s, s_tmp);
  if (threadIdx.x == 0) unit_sumsq[blockIdx.x] = s;
}

// one block per segment: fixed-order fold of its units -> norm, coef
__global__ void __launch_bounds__(256) seg_norm_kernel(const float* __restrict__ unit_sumsq, const int64_t* __restrict__ seg_off,
                                                       float clip, float* __restrict__ norms, float* __restrict__ coef) {
  __shared__ float s_tmp[4];
  const int sgi = blockIdx.x;
  const int64_t u0 = seg_off[sgi] / kUnit, u1 = seg_off[sgi + 1] / kUnit;
  float s = 0.f;
  for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) s += unit_sumsq[u];
  s = block_sum_256(s, s_tmp);
  if (threadIdx.x == 0) {
    const float n = sqrtf(s);
    norms[sgi] = n;
    float c = 1.0f;
    if (clip > 0.f) {
      const float cc = clip / (n + 1e-6f);  // misc.py:380
      if (cc < 1.0f) c = cc;                // misc.py:381
    }
    coef[sgi] = c;
  }
}

__device__ __forceinline__ int find_segment(const int64_t* __restrict__ seg_off, int nseg, int64_t pos) {
  int lo = 0, hi = nseg;  // seg_off[lo] <= pos < seg_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_off[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) scale_units_kernel(float* __restrict__ g, const int64_t* __restrict__ seg_off,
                                                          const float* __restrict__ coef, int nseg, int64_t total) {
  const int64_t base = (int64_t)blockIdx.x * kUnit;
  const float c = coef[find_segment(seg_off, nseg, base)];
  if (c == 1.0f) return;
  const int64_t i = base + threadIdx.x * 4;
  if (i < total) Vec4<float>::store(g + i, Vec4<float>::load(g + i) * c);
}

// Per-segment multipliers of the rate and of the decay (the *_scaled entry points; torch param groups in the reference,
// src/utils/optimizers.py:344-379).  A unit belongs to one segment, so lr_s = lr*lr_scale[s] and wd_s = wd*wd_scale[s] are
// block-uniform: each block forms its constants in double from the launch scalars and rounds once, where the host rounds for the
// unscaled kernels -- a scale of 1.0 is exact in double, so all-ones scales give the unscaled call's bits.  kScaled = false is the
// unscaled kernel: it never looks at this struct.
struct SegScales {
  const float* lr_scale;  // [nseg] or null = all ones
  const float* wd_scale;  // [nseg] or null = all ones
  double lr, wd;          // the launch scalars
  double bc1;             // AdamW: 1 - beta1^t
};

__device__ __forceinline__ double seg_lr(const SegScales& sc, int sgi) {
  return sc.lr_scale ? sc.lr * (double)sc.lr_scale[sgi] : sc.lr;
}

// lr_s * wd_s, grouped as the host groups lr * wd
__device__ __forceinline__ double seg_lr_wd(const SegScales& sc, int sgi, double lr_s) {
  const double x = lr_s * sc.wd;
  return sc.wd_scale ? x * (double)sc.wd_scale[sgi] : x;
}

struct AdamArgs {
  float lr_wd_keep;   // 1 - lr*wd
  float one_m_b1, b2, one_m_b2;
  float step_size;    // lr / (1 - b1^t)
  float inv_bc2_sqrt; // 1 / sqrt(1 - b2^t)
  float eps;
};

template <bool kScaled>
__global__ void __launch_bounds__(256) adamw_units_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, const int64_t* __restrict__ seg_off,
                                                          const float* __restrict__ coef, const uint8_t* __restrict__ skip,
                                                          int nseg, int64_t total, AdamArgs a, SegScales sc,
                                                          bf16* __restrict__ p_bf16) {
  const int64_t base = (int64_t)blockIdx.x * kUnit;
  const int sgi = find_segment(seg_off, nseg, base);
  const int64_t i = base + threadIdx.x * 4;
  if (i >= total) return;
  if (skip && skip[sgi]) return;
  const float c = coef ? coef[sgi] : 1.0f;
  if constexpr (kScaled) {
    const double lr_s = seg_lr(sc, sgi);
    a.lr_wd_keep = (float)(1.0 - seg_lr_wd(sc, sgi, lr_s));
    a.step_size = (float)(lr_s / sc.bc1);
  }
  // the fp32 parameter / gradient / moment streams are non-temporal (measured in the step: -0.17 ms); the bf16 weight copies, which
  // the next step's first GEMMs read, stay cacheable
  f32x4 gv = Vec4<float>::load_nt(g + i);
  if (c != 1.0f) {
    gv = gv * c;
    Vec4<float>::store(g + i, gv);  // leave the clipped gradient in .grad like the reference does
  }
  f32x4 pv = Vec4<float>::load_nt(p + i) * a.lr_wd_keep;          // param.mul_(1 - lr*wd)
  f32x4 mv = Vec4<float>::load_nt(m + i);
  mv = mv + (gv - mv) * a.one_m_b1;                            // exp_avg.lerp_(grad, 1-beta1)
  f32x4 vv = Vec4<float>::load_nt(v + i) * a.b2 + gv * gv * a.one_m_b2;
  f32x4 den;
#pragma unroll
  for (int e = 0; e < 4; ++e) den[e] = sqrtf(vv[e]) * a.inv_bc2_sqrt + a.eps;
#pragma unroll
  for (int e = 0; e < 4; ++e) pv[e] = pv[e] - a.step_size * (mv[e] / den[e]);
  Vec4<float>::store_nt(p + i, pv);
  Vec4<float>::store_nt(m + i, mv);
  Vec4<float>::store_nt(v + i, vv);
  if (p_bf16) Vec4<bf16>::store(p_bf16 + i, pv);
}

// torch.optim.AdamW counts steps per parameter: one that received no gradient (p.grad is None) is passed over, and its bias
// correction starts at 1 when it first receives one.  seg_step[s] is the 1-based number of the update this launch makes to segment
// s; each block forms the two corrections of its segment in double, as adamw_launch forms them on the host for a count shared by
// all segments, and rounds once.  lr_scale / wd_scale as in the scaled kernel (null = all ones).
struct SegSteps {
  const int32_t* seg_step;  // [nseg]; the entry of a skipped segment is not read
  double beta1, beta2;
};

__global__ void __launch_bounds__(256) adamw_counts_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, const int64_t* __restrict__ seg_off,
                                                           const float* __restrict__ coef, const uint8_t* __restrict__ skip,
                                                           int nseg, int64_t total, AdamArgs a, SegScales sc, SegSteps ss,
                                                           bf16* __restrict__ p_bf16) {
  const int64_t base = (int64_t)blockIdx.x * kUnit;
  const int sgi = find_segment(seg_off, nseg, base);
  const int64_t i = base + threadIdx.x * 4;
  if (i >= total) return;
  if (skip && skip[sgi]) return;
  const float c = coef ? coef[sgi] : 1.0f;
  const double t = (double)ss.seg_step[sgi];
  const double bc1 = 1.0 - pow(ss.beta1, t), bc2 = 1.0 - pow(ss.beta2, t);
  const double lr_s = seg_lr(sc, sgi);
  a.lr_wd_keep = (float)(1.0 - seg_lr_wd(sc, sgi, lr_s));
  a.step_size = (float)(lr_s / bc1);
  a.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
  // from here on the text of adamw_units_kernel, which stays as it was (its code object is the benchmarked step's)
  f32x4 gv = Vec4<float>::load_nt(g + i);
  if (c != 1.0f) {
    gv = gv * c;
    Vec4<float>::store(g + i, gv);  // leave the clipped gradient in .grad like the reference does
  }
  f32x4 pv = Vec4<float>::load_nt(p + i) * a.lr_wd_keep;          // param.mul_(1 - lr*wd)
  f32x4 mv = Vec4<float>::load_nt(m + i);
  mv = mv + (gv - mv) * a.one_m_b1;                            // exp_avg.lerp_(grad, 1-beta1)
  f32x4 vv = Vec4<float>::load_nt(v + i) * a.b2 + gv * gv * a.one_m_b2;
  f32x4 den;
#pragma unroll
  for (int e = 0; e < 4; ++e) den[e] = sqrtf(vv[e]) * a.inv_bc2_sqrt + a.eps;
#pragma unroll
  for (int e = 0; e < 4; ++e) pv[e] = pv[e] - a.step_size * (mv[e] / den[e]);
  Vec4<float>::store_nt(p + i, pv);
  Vec4<float>::store_nt(m + i, mv);
  Vec4<float>::store_nt(v + i, vv);
  if (p_bf16) Vec4<bf16>::store(p_bf16 + i, pv);
}

// ---- Lion / SGD / Lamb (src/utils/optimizers.py:267-279, torch.optim.SGD, optimizers.py:154-172) on the same unit layout and with the
// same conventions as adamw_units_kernel: deferred clip coefficient with the clipped gradient written back, per-segment skip mask
// (parameter AND state bits untouched), fp32 streams non-temporal, bf16 shadow cacheable.  No floating-point atomics anywhere.
struct LionArgs {
  float lr_wd_keep;  // 1 - lr*wd
  float lr, b1, one_m_b1, b2, one_m_b2;
};

template <bool kScaled>
__global__ void __launch_bounds__(256) lion_units_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                         const int64_t* __restrict__ seg_off, const float* __restrict__ coef,
                                                         const uint8_t* __restrict__ skip, int nseg, int64_t total, LionArgs a,
                                                         SegScales sc, bf16* __restrict__ p_bf16) {
  const int64_t base = (int64_t)blockIdx.x * kUnit;
  const int sgi = find_segment(seg_off, nseg, base);
  const int64_t i = base + threadIdx.x * 4;
  if (i >= total) return;
  if (skip && skip[sgi]) return;
  const float c = coef ? coef[sgi] : 1.0f;
  if constexpr (kScaled) {
    const double lr_s = seg_lr(sc, sgi);
    a.lr_wd_keep = (float)(1.0 - seg_lr_wd(sc, sgi, lr_s));
    a.lr = (float)lr_s;
  }
  f32x4 gv = Vec4<float>::load_nt(g + i);
  if (c != 1.0f) {
    gv = gv * c;
    Vec4<float>::store(g + i, gv);
  }
  f32x4 pv = Vec4<float>::load_nt(p + i) * a.lr_wd_keep;  // p.mul_(1 - lr*wd)
  f32x4 mv = Vec4<float>::load_nt(m + i);
  const f32x4 cv = mv * a.b1 + gv * a.one_m_b1;           // the moment BEFORE this step
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float sg = (float)(cv[e] > 0.f) - (float)(cv[e] < 0.f);  // sign(0) = 0
    pv[e] = pv[e] - a.lr * sg;
  }
  mv = mv * a.b2 + gv * a.one_m_b2;
  Vec4<float>::store_nt(p + i, pv);
  Vec4<float>::store_nt(m + i, mv);
  if (p_bf16) Vec4<bf16>::store(p_bf16 + i, pv);
}

// buf may be null (momentum == 0: torch keeps no buffer and the update is p - lr*g)
template <bool kScaled>
__global__ void __launch_bounds__(256) sgd_units_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf,
                                                        const int64_t* __restrict__ seg_off, const float* __restrict__ coef,
                                                        const uint8_t* __restrict__ skip, int nseg, int64_t total, float lr,
                                                        float momentum, SegScales sc, bf16* __restrict__ p_bf16) {
  const int64_t base = (int64_t)blockIdx.x * kUnit;
  const int sgi = find_segment(seg_off, nseg, base);
  const int64_t i = base + threadIdx.x * 4;
  if (i >= total) return;
  if (skip && skip[sgi]) return;
  const float c = coef ? coef[sgi] : 1.0f;
  if constexpr (kScaled) lr = (float)seg_lr(sc, sgi);
  f32x4 gv = Vec4<float>::load_nt(g + i);
  if (c != 1.0f) {
    gv = gv * c;
    Vec4<float>::store(g + i, gv);
  }
  f32x4 bv = gv;
  if (buf) {
    bv = Vec4<float>::load_nt(buf + i) * momentum + gv;  // buf.mul_(momentum).add_(g); a zero buffer gives the first step's buf = g
    Vec4<float>::store_nt(buf + i, bv);
  }
  const f32x4 pv = Vec4<float>::load_nt(p + i) - bv * lr;
  Vec4<float>::store_nt(p + i, pv);
  if (p_bf16) Vec4<bf16>::store(p_bf16 + i, pv);
}

struct LambArgs {
  float lr, b1, one_m_b1, b2, one_m_b2, eps, wd;
};

// adam_step of one element.  The update pass calls it on the moments the first pass stored, so the u it steps by is the u whose
// norm went into the trust ratio (the library is built without floating-point contraction, build.py).
__device__ __forceinline__ float lamb_u(float m, float v, float p, float eps, float wd) {
  return m / (sqrtf(v) + eps) + wd * p;
}

// wd_s as a float: the update pass must step by the u whose norm the moments pass took
__device__ __forceinline__ float seg_wd(const SegScales& sc, int sgi) {
  return (float)(sc.wd_scale ? sc.wd * (double)sc.wd_scale[sgi] : sc.wd);
}

// (a) moments + the two per-unit partial sums  unit_sums[2*unit] = sum p^2, [2*unit + 1] = sum u^2
template <bool kScaled>
__global__ void __launch_bounds__(256) lamb_moments_kernel(const float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, const int64_t* __restrict__ seg_off,
                                                           const float* __restrict__ coef, const uint8_t* __restrict__ skip,
                                                           int nseg, int64_t total, LambArgs a, SegScales sc,
                                                           float* __restrict__ unit_sums) {
  __shared__ float s_tmp[4];
  const int64_t base = (int64_t)blockIdx.x * kUnit;
  const int sgi = find_segment(seg_off, nseg, base);
  if (skip && skip[sgi]) return;  // block-uniform: a unit belongs to one segment
  if constexpr (kScaled) a.wd = seg_wd(sc, sgi);
  const int64_t i = base + threadIdx.x * 4;
  float sp = 0.f, su = 0.f;
  if (i < total) {
    const float c = coef ? coef[sgi] : 1.0f;
    f32x4 gv = Vec4<float>::load_nt(g + i);
    if (c != 1.0f) {
      gv = gv * c;
      Vec4<float>::store(g + i, gv);
    }
    const f32x4 pv = Vec4<float>::load_nt(p + i);
    const f32x4 mv = Vec4<float>::load_nt(m + i) * a.b1 + gv * a.one_m_b1;
    const f32x4 vv = Vec4<float>::load_nt(v + i) * a.b2 + (gv * gv) * a.one_m_b2;
    Vec4<float>::store_nt(m + i, mv);
    Vec4<float>::store_nt(v + i, vv);
    f32x4 uv;
#pragma unroll
    for (int e = 0; e < 4; ++e) uv[e] = lamb_u(mv[e], vv[e], pv[e], a.eps, a.wd);
    sp = (pv[0] * pv[0] + pv[1] * pv[1]) + (pv[2] * pv[2] + pv[3] * pv[3]);
    su = (uv[0] * uv[0] + uv[1] * uv[1]) + (uv[2] * uv[2] + uv[3] * uv[3]);
  }
  sp = block_sum_256(sp, s_tmp);
  su = block_sum_256(su, s_tmp);
  if (threadIdx.x == 0) {
    unit_sums[2 * (int64_t)blockIdx.x] = sp;
    unit_sums[2 * (int64_t)blockIdx.x + 1] = su;
  }
}

// (b) one block per segment: fixed-order fold of its units -> weight_norm = min(||p||, 10), adam_norm = ||u||, trust_ratio
__global__ void __launch_bounds__(256) lamb_trust_kernel(const float* __restrict__ unit_sums, const int64_t* __restrict__ seg_off,
                                                         const uint8_t* __restrict__ skip, float eps, float* __restrict__ weight_norm,
                                                         float* __restrict__ adam_norm, float* __restrict__ trust_ratio) {
  __shared__ float s_tmp[4];
  const int sgi = blockIdx.x;
  if (skip && skip[sgi]) return;  // a skipped segment keeps its diagnostics
  const int64_t u0 = seg_off[sgi] / kUnit, u1 = seg_off[sgi + 1] / kUnit;
  float sp = 0.f, su = 0.f;
  for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
    sp += unit_sums[2 * u];
    su += unit_sums[2 * u + 1];
  }
  sp = block_sum_256(sp, s_tmp);
  su = block_sum_256(su, s_tmp);
  if (threadIdx.x == 0) {
    const float w = fminf(sqrtf(sp), 10.0f);  // optimizers.py:163
    const float an = sqrtf(su);
    weight_norm[sgi] = w;
    adam_norm[sgi] = an;
    trust_ratio[sgi] = (w == 0.0f || an == 0.0f) ? 1.0f : w / (an + eps);  // optimizers.py:166-168
  }
}

// (c) update: u recomputed from the moments pass (a) wrote
template <bool kScaled>
__global__ void __launch_bounds__(256) lamb_update_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                          const int64_t* __restrict__ seg_off, const uint8_t* __restrict__ skip,
                                                          int nseg, int64_t total, LambArgs a, SegScales sc,
                                                          const float* __restrict__ trust_ratio, bf16* __restrict__ p_bf16) {
  const int64_t base = (int64_t)blockIdx.x * kUnit;
  const int sgi = find_segment(seg_off, nseg, base);
  const int64_t i = base + threadIdx.x * 4;
  if (i >= total) return;
  if (skip && skip[sgi]) return;
  if constexpr (kScaled) {
    a.lr = (float)seg_lr(sc, sgi);
    a.wd = seg_wd(sc, sgi);
  }
  const float sr = a.lr * trust_ratio[sgi];  // step_size * trust_ratio, optimizers.py:171
  f32x4 pv = Vec4<float>::load_nt(p + i);
  const f32x4 mv = Vec4<float>::load_nt(m + i), vv = Vec4<float>::load_nt(v + i);
#pragma unroll
  for (int e = 0; e < 4; ++e) pv[e] = pv[e] - sr * lamb_u(mv[e], vv[e], pv[e], a.eps, a.wd);
  Vec4<float>::store_nt(p + i, pv);
  if (p_bf16) Vec4<bf16>::store(p_bf16 + i, pv);
}

}  // namespace hct

using namespace hct;

extern "C" {

size_t hct_grad_norms_workspace_bytes(int64_t total) { return (size_t)((total + kUnit - 1) / kUnit) * sizeof(float); }

int hct_grad_norms(float* grads, const int64_t* seg_off, int nseg, int64_t total, float clip, int scale_in_place,
                   float* norms, float* coef, void* workspace, size_t workspace_bytes, void* stream) {
  HCT_REQUIRE(total > 0 && total % kUnit == 0 && nseg > 0, "hct_grad_norms: total must be a positive multiple of %d", kUnit);
  if (workspace_bytes < hct_grad_norms_workspace_bytes(total)) {
    set_error("hct_grad_norms: workspace too small");
    return HCT_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const int units = (int)(total / kUnit);
  hipLaunchKernelGGL(sumsq_units_kernel, dim3(units), dim3(256), 0, s, grads, total, (float*)workspace);
  hipLaunchKernelGGL(seg_norm_kernel, dim3(nseg), dim3(256), 0, s, (const float*)workspace, seg_off, clip, norms, coef);
  if (scale_in_place && clip > 0.f)
    hipLaunchKernelGGL(scale_units_kernel, dim3(units), dim3(256), 0, s, grads, seg_off, coef, nseg, total);
  HCT_CHECK_LAUNCH("hct_grad_norms");
  return 0;
}

static int adamw_launch(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off, const float* coef,
                        const uint8_t* skip, int nseg, int64_t total, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, void* params_bf16, const float* lr_scale, const float* wd_scale, void* stream,
                        const char* who) {
  HCT_REQUIRE(total > 0 && total % kUnit == 0 && nseg > 0 && step >= 1, "%s: bad arguments", who);
  AdamArgs a;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  a.lr_wd_keep = (float)(1.0 - (double)lr * (double)weight_decay);
  a.one_m_b1 = (float)(1.0 - (double)beta1);
  a.b2 = beta2;
  a.one_m_b2 = (float)(1.0 - (double)beta2);
  a.step_size = (float)((double)lr / bc1);
  a.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
  a.eps = eps;
  const SegScales sc{lr_scale, wd_scale, (double)lr, (double)weight_decay, bc1};
  const dim3 grid((int)(total / kUnit));
  if (lr_scale || wd_scale)
    hipLaunchKernelGGL(adamw_units_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, seg_off,
                       coef, skip, nseg, total, a, sc, (bf16*)params_bf16);
  else
    hipLaunchKernelGGL(adamw_units_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, seg_off,
                       coef, skip, nseg, total, a, sc, (bf16*)params_bf16);
  HCT_CHECK_LAUNCH(who);
  return 0;
}

int hct_adamw_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off,
                   const float* coef, const uint8_t* skip, int nseg, int64_t total, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int step, void* params_bf16, void* stream) {
  return adamw_launch(params, grads, exp_avg, exp_avg_sq, seg_off, coef, skip, nseg, total, lr, beta1, beta2, eps, weight_decay, step,
                      params_bf16, nullptr, nullptr, stream, "hct_adamw_step");
}

int hct_adamw_step_scaled(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off,
                          const float* coef, const uint8_t* skip, int nseg, int64_t total, float lr, float beta1, float beta2,
                          float eps, float weight_decay, int step, void* params_bf16, const float* lr_scale,
                          const float* wd_scale, void* stream) {
  return adamw_launch(params, grads, exp_avg, exp_avg_sq, seg_off, coef, skip, nseg, total, lr, beta1, beta2, eps, weight_decay, step,
                      params_bf16, lr_scale, wd_scale, stream, "hct_adamw_step_scaled");
}

int hct_adamw_step_counts(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off,
                          const float* coef, const uint8_t* skip, int nseg, int64_t total, float lr, float beta1, float beta2,
                          float eps, float weight_decay, const int32_t* seg_step, void* params_bf16, const float* lr_scale,
                          const float* wd_scale, void* stream) {
  HCT_REQUIRE(params && grads && exp_avg && exp_avg_sq && seg_off && seg_step && total > 0 && total % kUnit == 0 && nseg > 0,
              "hct_adamw_step_counts: bad arguments");
  AdamArgs a;
  a.lr_wd_keep = 1.0f;  // the three that depend on the segment are formed by each block
  a.step_size = 0.0f;
  a.inv_bc2_sqrt = 1.0f;
  a.one_m_b1 = (float)(1.0 - (double)beta1);
  a.b2 = beta2;
  a.one_m_b2 = (float)(1.0 - (double)beta2);
  a.eps = eps;
  const SegScales sc{lr_scale, wd_scale, (double)lr, (double)weight_decay, 1.0};
  const SegSteps ss{seg_step, (double)beta1, (double)beta2};
  hipLaunchKernelGGL(adamw_counts_kernel, dim3((int)(total / kUnit)), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg,
                     exp_avg_sq, seg_off, coef, skip, nseg, total, a, sc, ss, (bf16*)params_bf16);
  HCT_CHECK_LAUNCH("hct_adamw_step_counts");
  return 0;
}

static int lion_launch(float* params, float* grads, float* exp_avg, const int64_t* seg_off, const float* coef, const uint8_t* skip,
                       int nseg, int64_t total, double lr, double beta1, double beta2, double weight_decay, void* params_bf16,
                       const float* lr_scale, const float* wd_scale, void* stream, const char* who) {
  HCT_REQUIRE(params && grads && exp_avg && seg_off && total > 0 && total % kUnit == 0 && nseg > 0, "%s: bad arguments", who);
  LionArgs a;
  a.lr_wd_keep = (float)(1.0 - lr * weight_decay);
  a.lr = (float)lr;
  a.b1 = (float)beta1;
  a.one_m_b1 = (float)(1.0 - beta1);
  a.b2 = (float)beta2;
  a.one_m_b2 = (float)(1.0 - beta2);
  const SegScales sc{lr_scale, wd_scale, lr, weight_decay, 1.0};
  const dim3 grid((int)(total / kUnit));
  if (lr_scale || wd_scale)
    hipLaunchKernelGGL(lion_units_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, seg_off, coef, skip,
                       nseg, total, a, sc, (bf16*)params_bf16);
  else
    hipLaunchKernelGGL(lion_units_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, seg_off, coef, skip,
                       nseg, total, a, sc, (bf16*)params_bf16);
  HCT_CHECK_LAUNCH(who);
  return 0;
}

int hct_lion_step(float* params, float* grads, float* exp_avg, const int64_t* seg_off, const float* coef, const uint8_t* skip,
                  int nseg, int64_t total, double lr, double beta1, double beta2, double weight_decay, void* params_bf16,
                  void* stream) {
  return lion_launch(params, grads, exp_avg, seg_off, coef, skip, nseg, total, lr, beta1, beta2, weight_decay, params_bf16, nullptr,
                     nullptr, stream, "hct_lion_step");
}

int hct_lion_step_scaled(float* params, float* grads, float* exp_avg, const int64_t* seg_off, const float* coef, const uint8_t* skip,
                         int nseg, int64_t total, double lr, double beta1, double beta2, double weight_decay, void* params_bf16,
                         const float* lr_scale, const float* wd_scale, void* stream) {
  return lion_launch(params, grads, exp_avg, seg_off, coef, skip, nseg, total, lr, beta1, beta2, weight_decay, params_bf16, lr_scale,
                     wd_scale, stream, "hct_lion_step_scaled");
}

static int sgd_launch(float* params, float* grads, float* momentum_buf, const int64_t* seg_off, const float* coef, const uint8_t* skip,
                      int nseg, int64_t total, double lr, double momentum, void* params_bf16, const float* lr_scale, void* stream,
                      const char* who) {
  HCT_REQUIRE(params && grads && seg_off && total > 0 && total % kUnit == 0 && nseg > 0, "%s: bad arguments", who);
  HCT_REQUIRE(momentum_buf || momentum == 0.0, "%s: momentum %g needs a momentum buffer", who, momentum);
  const SegScales sc{lr_scale, nullptr, lr, 0.0, 1.0};
  const dim3 grid((int)(total / kUnit));
  float* buf = momentum == 0.0 ? (float*)nullptr : momentum_buf;
  if (lr_scale)
    hipLaunchKernelGGL(sgd_units_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, params, grads, buf, seg_off, coef, skip, nseg,
                       total, (float)lr, (float)momentum, sc, (bf16*)params_bf16);
  else
    hipLaunchKernelGGL(sgd_units_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, params, grads, buf, seg_off, coef, skip, nseg,
                       total, (float)lr, (float)momentum, sc, (bf16*)params_bf16);
  HCT_CHECK_LAUNCH(who);
  return 0;
}

int hct_sgd_step(float* params, float* grads, float* momentum_buf, const int64_t* seg_off, const float* coef, const uint8_t* skip,
                 int nseg, int64_t total, double lr, double momentum, void* params_bf16, void* stream) {
  return sgd_launch(params, grads, momentum_buf, seg_off, coef, skip, nseg, total, lr, momentum, params_bf16, nullptr, stream,
                    "hct_sgd_step");
}

int hct_sgd_step_scaled(float* params, float* grads, float* momentum_buf, const int64_t* seg_off, const float* coef,
                        const uint8_t* skip, int nseg, int64_t total, double lr, double momentum, void* params_bf16,
                        const float* lr_scale, void* stream) {
  return sgd_launch(params, grads, momentum_buf, seg_off, coef, skip, nseg, total, lr, momentum, params_bf16, lr_scale, stream,
                    "hct_sgd_step_scaled");
}

size_t hct_lamb_workspace_bytes(int64_t total, int nseg) {
  (void)nseg;
  return (size_t)((total + kUnit - 1) / kUnit) * 2 * sizeof(float);
}

static int lamb_launch(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off, const float* coef,
                       const uint8_t* skip, int nseg, int64_t total, double lr, double beta1, double beta2, double eps,
                       double weight_decay, float* weight_norm, float* adam_norm, float* trust_ratio, void* workspace,
                       size_t workspace_bytes, void* params_bf16, const float* lr_scale, const float* wd_scale, void* stream,
                       const char* who) {
  HCT_REQUIRE(params && grads && exp_avg && exp_avg_sq && seg_off && weight_norm && adam_norm && trust_ratio && total > 0 &&
                  total % kUnit == 0 && nseg > 0,
              "%s: bad arguments", who);
  if (!workspace || workspace_bytes < hct_lamb_workspace_bytes(total, nseg)) {
    set_error("%s: workspace too small", who);
    return HCT_E_WORKSPACE;
  }
  LambArgs a;
  a.lr = (float)lr;
  a.b1 = (float)beta1;
  a.one_m_b1 = (float)(1.0 - beta1);
  a.b2 = (float)beta2;
  a.one_m_b2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  a.wd = (float)weight_decay;
  const SegScales sc{lr_scale, wd_scale, lr, weight_decay, 1.0};
  hipStream_t s = (hipStream_t)stream;
  const int units = (int)(total / kUnit);
  if (wd_scale)  // the moments pass uses no rate
    hipLaunchKernelGGL(lamb_moments_kernel<true>, dim3(units), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, seg_off, coef, skip,
                       nseg, total, a, sc, (float*)workspace);
  else
    hipLaunchKernelGGL(lamb_moments_kernel<false>, dim3(units), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, seg_off, coef, skip,
                       nseg, total, a, sc, (float*)workspace);
  hipLaunchKernelGGL(lamb_trust_kernel, dim3(nseg), dim3(256), 0, s, (const float*)workspace, seg_off, skip, a.eps, weight_norm,
                     adam_norm, trust_ratio);
  if (lr_scale || wd_scale)
    hipLaunchKernelGGL(lamb_update_kernel<true>, dim3(units), dim3(256), 0, s, params, exp_avg, exp_avg_sq, seg_off, skip, nseg, total,
                       a, sc, trust_ratio, (bf16*)params_bf16);
  else
    hipLaunchKernelGGL(lamb_update_kernel<false>, dim3(units), dim3(256), 0, s, params, exp_avg, exp_avg_sq, seg_off, skip, nseg, total,
                       a, sc, trust_ratio, (bf16*)params_bf16);
  HCT_CHECK_LAUNCH(who);
  return 0;
}

int hct_lamb_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off, const float* coef,
                  const uint8_t* skip, int nseg, int64_t total, double lr, double beta1, double beta2, double eps,
                  double weight_decay, float* weight_norm, float* adam_norm, float* trust_ratio, void* workspace,
                  size_t workspace_bytes, void* params_bf16, void* stream) {
  return lamb_launch(params, grads, exp_avg, exp_avg_sq, seg_off, coef, skip, nseg, total, lr, beta1, beta2, eps, weight_decay,
                     weight_norm, adam_norm, trust_ratio, workspace, workspace_bytes, params_bf16, nullptr, nullptr, stream,
                     "hct_lamb_step");
}

int hct_lamb_step_scaled(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off, const float* coef,
                         const uint8_t* skip, int nseg, int64_t total, double lr, double beta1, double beta2, double eps,
                         double weight_decay, float* weight_norm, float* adam_norm, float* trust_ratio, void* workspace,
                         size_t workspace_bytes, void* params_bf16, const float* lr_scale, const float* wd_scale, void* stream) {
  return lamb_launch(params, grads, exp_avg, exp_avg_sq, seg_off, coef, skip, nseg, total, lr, beta1, beta2, eps, weight_decay,
                     weight_norm, adam_norm, trust_ratio, workspace, workspace_bytes, params_bf16, lr_scale, wd_scale, stream,
                     "hct_lamb_step_scaled");
}

}  // extern "C"
