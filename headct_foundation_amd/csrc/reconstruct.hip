// Inference side of a trained masked autoencoder: reconstructions and per-patch error maps accumulated over a schedule of masks
// (headct_foundation_amd/reconstruct.py).
//
// hct_mae_recon_accum: one workgroup of 256 threads per prediction row (b, t), as masked_mse_kernel; the class row and the rows
// of kept patches (mask == 0) leave after one scalar load.  For a masked patch the block
//   1. with norm_pix, reads the patch of x twice for mean and unbiased variance (two fixed-order block sums, the arithmetic of
//      masked_mse_kernel: mu = sum / pd, var = sum (t - mu)^2 / (pd - 1), sd = sqrt(var + 1e-6));
//   2. walks the patch in "quads": four consecutive voxels along the last volume axis (P % 4 == 0, so a quad never leaves its
//      patch) times the C channels.  In the prediction row a quad is 4 C CONTIGUOUS elements (channel fastest), read as C
//      vectors of four (8 bytes bf16 / 16 bytes fp32 per lane); in the volume it is one vector of four per channel (x: 8 bytes
//      fp16 / 16 bytes fp32; recon_sum: 16 bytes).  The channel interleave is undone in registers, which needs C at compile
//      time: C = 1 ... 4 are instantiated, a larger C runs the same loop with scalar reads of the prediction;
//   3. writes v = pred sd + mu over (count == 0) or onto (count > 0) the patch's voxels of recon_sum, and the patch's
//      e = mean_k (pred_k - target_k)^2 -- the per-patch term of the loss, in loss units -- into err_sum the same way.
// Every element of recon_sum / err_sum / cnt has exactly one writer per launch, a thread adds its quads in ascending order and
// the block sums run in a fixed order: no atomics, a repeated sequence of calls is bit-identical.  pred, the last read of x and
// recon_sum are touched once per launch and use the non-temporal policy.
//
// hct_mae_recon_finish: one workgroup per patch: recon = cnt ? recon_sum / cnt : x, err = cnt ? err_sum / cnt : 0, and
// optionally err_vol [B, S, S, S] = err of the voxel's patch.  recon may alias recon_sum (every quad is read and written by one thread).
#include <math.h>

#include "common.h"

using namespace hct;

namespace {

__device__ __forceinline__ float block_sum_256(float v, float* s_tmp) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_tmp[0] + s_tmp[1]) + (s_tmp[2] + s_tmp[3]);
}

// where patch l of volume b starts, and how a quad index q < P^3 / 4 maps to a voxel offset inside one channel of the volume
struct PatchGeom {
  int S, P, P4;       // P4 = P / 4 quads along the last axis
  size_t origin;      // voxel offset of the patch's corner inside a channel
  __device__ __forceinline__ PatchGeom(int S_, int P_, int l) : S(S_), P(P_), P4(P_ / 4) {
    const int g = S / P;
    const int gh = l / (g * g), gw = (l / g) % g, gd = l % g;
    origin = ((size_t)(gh * P) * S + gw * P) * S + gd * P;
  }
  __device__ __forceinline__ size_t voxel(int q) const {  // q = (ph * P + pw) * P4 + pz / 4
    const int z4 = q % P4;
    const int u = q / P4;
    const int pw = u % P, ph = u / P;
    return origin + ((size_t)ph * S + pw) * S + z4 * 4;
  }
};

// the 4 C prediction values of a quad as out[c][e] (voxel e of the quad, channel c); p points at the quad's first element
template <int CT, typename T>
__device__ __forceinline__ void load_pred_quad(const T* p, int C, f32x4* out) {
  if constexpr (CT > 0) {
    f32x4 raw[CT];
#pragma unroll
    for (int i = 0; i < CT; ++i) raw[i] = Vec4<T>::load_nt(p + 4 * i);
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) out[c][e] = raw[(e * CT + c) / 4][(e * CT + c) % 4];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) out[0][e] = to_f32(p[e * C]);  // (generic C: the caller passes p + c and takes out[0])
  }
}

template <int CT, typename TX, typename T>
__global__ void __launch_bounds__(256) mae_recon_accum_kernel(const T* __restrict__ pred, int has_cls, const TX* __restrict__ x,
                                                              const float* __restrict__ mask, int C, int S, int P, int L, int norm_pix,
                                                              float* __restrict__ recon_sum, float* __restrict__ err_sum,
                                                              int32_t* __restrict__ cnt) {
  __shared__ float s_tmp[4];
  const int r = blockIdx.x;
  const int rows = L + has_cls;
  const int b = r / rows, t = r - b * rows;
  if (t < has_cls) return;  // class row
  const int l = t - has_cls;
  const size_t slot = (size_t)b * L + l;
  if (mask[slot] == 0.f) return;  // kept patch: nothing is read or written
  const int seen = cnt[slot];     // (every thread reads it before the first barrier; thread 0 writes it after the last)
  const int nc = CT > 0 ? CT : C;
  const int pd = P * P * P * nc;
  const int nq = P * P * (P / 4);
  const size_t chan = (size_t)S * S * S;
  const PatchGeom geo(S, P, l);
  const T* prow = pred + (size_t)r * pd;
  const TX* vol = x + (size_t)b * nc * chan;
  float* rvol = recon_sum + (size_t)b * nc * chan;

  float mu = 0.f, sd = 1.f, rsd = 1.f;
  if (norm_pix) {
    float s = 0.f;
    for (int q = threadIdx.x; q < nq; q += 256) {
      const size_t v = geo.voxel(q);
      for (int c = 0; c < nc; ++c) {
        const f32x4 tv = Vec4<TX>::load(vol + c * chan + v);
        s += (tv[0] + tv[1]) + (tv[2] + tv[3]);
      }
    }
    mu = block_sum_256(s, s_tmp) / (float)pd;
    float ss = 0.f;
    for (int q = threadIdx.x; q < nq; q += 256) {
      const size_t v = geo.voxel(q);
      for (int c = 0; c < nc; ++c) {
        const f32x4 d = Vec4<TX>::load(vol + c * chan + v) - mu;
        ss += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
      }
    }
    const float var = block_sum_256(ss, s_tmp) / (float)(pd - 1);  // unbiased, mae.py:292
    sd = sqrtf(var + 1.0e-6f);
    rsd = 1.0f / sd;
  }

  float sse = 0.f;
  for (int q = threadIdx.x; q < nq; q += 256) {
    const size_t v = geo.voxel(q);
    const T* pq = prow + (size_t)q * 4 * nc;
    f32x4 pv[CT > 0 ? CT : 1];
    if constexpr (CT > 0) load_pred_quad<CT, T>(pq, nc, pv);
    for (int c = 0; c < nc; ++c) {
      if constexpr (CT == 0) load_pred_quad<0, T>(pq + c, nc, pv);
      const f32x4 p = pv[CT > 0 ? c : 0];
      const f32x4 tgt = (Vec4<TX>::load_nt(vol + c * chan + v) - mu) * rsd;
      const f32x4 df = p - tgt;
      sse += (df[0] * df[0] + df[1] * df[1]) + (df[2] * df[2] + df[3] * df[3]);
      f32x4 out = p * sd + mu;
      float* rp = rvol + c * chan + v;
      if (seen) out += Vec4<float>::load_nt(rp);
      Vec4<float>::store_nt(rp, out);
    }
  }
  sse = block_sum_256(sse, s_tmp);
  if (threadIdx.x == 0) {
    const float e = sse / (float)pd;
    err_sum[slot] = seen ? err_sum[slot] + e : e;
    cnt[slot] = seen + 1;
  }
}

// recon / recon_sum may be the same buffer: no __restrict__ on them
template <typename TX>
__global__ void __launch_bounds__(256) mae_recon_finish_kernel(const float* recon_sum, const float* __restrict__ err_sum,
                                                               const int32_t* __restrict__ cnt, const TX* __restrict__ x, int C, int S, int P,
                                                               int L, float* recon, float* __restrict__ err, float* __restrict__ err_vol) {
  const int r = blockIdx.x;
  const int b = r / L, l = r - b * L;
  const int n = cnt[r];
  const float e = n ? err_sum[r] / (float)n : 0.f;
  const int nq = P * P * (P / 4);
  const size_t chan = (size_t)S * S * S;
  const PatchGeom geo(S, P, l);
  for (int q = threadIdx.x; q < nq; q += 256) {
    const size_t v = geo.voxel(q);
    for (int c = 0; c < C; ++c) {
      const size_t at = ((size_t)b * C + c) * chan + v;
      const f32x4 out = n ? Vec4<float>::load_nt(recon_sum + at) / (float)n : Vec4<TX>::load_nt(x + at);
      Vec4<float>::store_nt(recon + at, out);
    }
    if (err_vol) Vec4<float>::store_nt(err_vol + (size_t)b * chan + v, f32x4{e, e, e, e});
  }
  if (threadIdx.x == 0) err[r] = e;
}

int check_geometry(const char* who, int B, int C, int S, int P, int x_dtype) {
  HCT_REQUIRE(B > 0 && C > 0 && S > 0 && P > 0, "%s: bad shape (B %d, C %d, S %d, P %d)", who, B, C, S, P);
  HCT_REQUIRE(P % 4 == 0 && S % P == 0, "%s: bad geometry S=%d P=%d (P %% 4 == 0 and S %% P == 0 are required)", who, S, P);
  HCT_REQUIRE(((int64_t)P * P * P * C) % 4 == 0, "%s: patch dim %% 4 != 0", who);
  HCT_REQUIRE(x_dtype == HCT_F32 || x_dtype == HCT_F16, "%s: volumes are fp32 or fp16", who);
  const int64_t g = S / P;
  HCT_REQUIRE((int64_t)B * (g * g * g + 1) < (1ll << 31), "%s: B * (L + 1) must fit a grid dimension", who);
  return 0;
}

template <typename TX, typename T>
void launch_accum(const void* pred, int has_cls, const void* x, const float* mask, int B, int C, int S, int P, int L, int norm_pix, float* recon_sum,
                  float* err_sum, int32_t* cnt, hipStream_t s) {
  const dim3 grid(B * (L + has_cls)), block(256);
#define HCT_RECON_LAUNCH(CT)                                                                                                                  \
  hipLaunchKernelGGL((mae_recon_accum_kernel<CT, TX, T>), grid, block, 0, s, (const T*)pred, has_cls, (const TX*)x, mask, C, S, P, L, norm_pix, \
                     recon_sum, err_sum, cnt)
  switch (C) {
    case 1: HCT_RECON_LAUNCH(1); break;
    case 2: HCT_RECON_LAUNCH(2); break;
    case 3: HCT_RECON_LAUNCH(3); break;
    case 4: HCT_RECON_LAUNCH(4); break;
    default: HCT_RECON_LAUNCH(0); break;
  }
#undef HCT_RECON_LAUNCH
}

}  // namespace

extern "C" {

int hct_mae_recon_accum(const void* pred, int pred_dtype, int has_cls_row, const void* x, int x_dtype, const float* mask, int B, int C, int S, int P,
                        int norm_pix, float* recon_sum, float* err_sum, int32_t* cnt, void* stream) {
  if (int rc = check_geometry("hct_mae_recon_accum", B, C, S, P, x_dtype)) return rc;
  HCT_REQUIRE(pred_dtype == HCT_F32 || pred_dtype == HCT_BF16, "hct_mae_recon_accum: pred must be HCT_F32 or HCT_BF16");
  HCT_REQUIRE(pred && x && mask && recon_sum && err_sum && cnt, "hct_mae_recon_accum: null argument");
  HCT_REQUIRE((((uintptr_t)pred | (uintptr_t)x | (uintptr_t)recon_sum) & 15) == 0, "hct_mae_recon_accum: pred, x and recon_sum must be 16-byte aligned");
  const int g = S / P, L = g * g * g;
  const int cls = has_cls_row ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  if (x_dtype == HCT_F16)
    HCT_DISPATCH_DTYPE(pred_dtype, T, (launch_accum<f16, T>(pred, cls, x, mask, B, C, S, P, L, norm_pix, recon_sum, err_sum, cnt, s)));
  else
    HCT_DISPATCH_DTYPE(pred_dtype, T, (launch_accum<float, T>(pred, cls, x, mask, B, C, S, P, L, norm_pix, recon_sum, err_sum, cnt, s)));
  return check_hip(hipGetLastError(), "hct_mae_recon_accum");
}

int hct_mae_recon_finish(const float* recon_sum, const float* err_sum, const int32_t* cnt, const void* x, int x_dtype, int B, int C, int S, int P,
                         float* recon, float* err, float* err_vol, void* stream) {
  if (int rc = check_geometry("hct_mae_recon_finish", B, C, S, P, x_dtype)) return rc;
  HCT_REQUIRE(recon_sum && err_sum && cnt && x && recon && err, "hct_mae_recon_finish: null argument");
  HCT_REQUIRE((((uintptr_t)recon_sum | (uintptr_t)x | (uintptr_t)recon | (uintptr_t)err_vol) & 15) == 0,
              "hct_mae_recon_finish: recon_sum, x, recon and err_vol must be 16-byte aligned");
  const int g = S / P, L = g * g * g;
  const dim3 grid(B * L), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (x_dtype == HCT_F16)
    hipLaunchKernelGGL(mae_recon_finish_kernel<f16>, grid, block, 0, s, recon_sum, err_sum, cnt, (const f16*)x, C, S, P, L, recon, err, err_vol);
  else
    hipLaunchKernelGGL(mae_recon_finish_kernel<float>, grid, block, 0, s, recon_sum, err_sum, cnt, (const float*)x, C, S, P, L, recon, err, err_vol);
  return check_hip(hipGetLastError(), "hct_mae_recon_finish");
}

}  // extern "C"
