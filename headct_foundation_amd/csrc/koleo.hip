// KoLeo regulariser (DINOv2 `KoLeoLoss`) on the class-token features x [n, D] of one global crop, per rank:
//   xh_i = x_i / max(||x_i||, 1e-8)                                   (F.normalize, eps 1e-8)
//   I_i  = argmax_{j != i} xh_i . xh_j                                 (lowest index on ties; a constant in the backward)
//   d_i  = || xh_i - xh_{I_i} + 1e-8 ||_2                              (F.pairwise_distance: the eps goes on every component)
//   loss = - mean_i log(d_i + 1e-8)
//   d loss / d xh_i = G_i - sum_{j: I_j = i} G_j,   G_i = - dloss / (n (d_i + 1e-8) d_i) * (xh_i - xh_{I_i} + 1e-8)
//   d loss / d x_i  = (dxh_i - xh_i (xh_i . dxh_i)) / ||x_i||
// Rows are read with a row stride, so the class-token rows of a [n, T, D] token tensor are used where they lie.  All arithmetic is
// fp32.  n = 64, D = 768 is 3 M multiply-adds: one workgroup per row, one wave per candidate, no MFMA; every sum is taken in a fixed
// order (the rows that chose row i are gathered by the block of row i, in row order: no atomics).
#include "common.h"

namespace hct {
namespace {

constexpr float kKoleoEps = 1e-8f;

// sum over the block's 256 threads, the same value in every thread (s_red: 4 floats; reusable after the call)
__device__ __forceinline__ float block_sum4(float v, float* s_red) {
  v = wave_sum(v);
  __syncthreads();  // (s_red may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// one block per row i; dynamic LDS: D floats (xh_i)
template <typename T>
__global__ void __launch_bounds__(256) koleo_fwd_kernel(const T* __restrict__ x, int n, int D, int64_t ldx, int32_t* __restrict__ nn_index,
                                                        float* __restrict__ dist, float* __restrict__ inv_norm) {
  extern __shared__ __attribute__((aligned(16))) float s_xi[];
  __shared__ float s_red[4];
  __shared__ float s_best[4], s_binv[4];
  __shared__ int s_bidx[4];
  const int i = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const T* xi = x + (size_t)i * ldx;
  float ss = 0.f;
  for (int k = threadIdx.x * 4; k < D; k += 1024) {
    const f32x4 v = Vec4<T>::load(xi + k);
    ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  ss = block_sum4(ss, s_red);
  const float inv_i = 1.0f / fmaxf(sqrtf(ss), kKoleoEps);
  for (int k = threadIdx.x * 4; k < D; k += 1024) *reinterpret_cast<f32x4*>(s_xi + k) = Vec4<T>::load(xi + k) * inv_i;
  __syncthreads();
  // wave w takes the candidates j = w, w + 4, ...: xh_i . xh_j and ||x_j|| from one read of row j
  float best = -INFINITY, best_inv = 0.f;
  int best_j = 0x7fffffff;
  for (int j = wave; j < n; j += 4) {
    if (j == i) continue;
    const T* xj = x + (size_t)j * ldx;
    float dot = 0.f, sj = 0.f;
    for (int k = lane * 4; k < D; k += 256) {
      const f32x4 v = Vec4<T>::load(xj + k), a = *reinterpret_cast<const f32x4*>(s_xi + k);
      dot += (a[0] * v[0] + a[1] * v[1]) + (a[2] * v[2] + a[3] * v[3]);
      sj += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    dot = wave_sum(dot);
    sj = wave_sum(sj);
    const float inv_j = 1.0f / fmaxf(sqrtf(sj), kKoleoEps);
    dot *= inv_j;
    if (dot > best) { best = dot; best_j = j; best_inv = inv_j; }  // ascending j: the lowest index keeps a tie
  }
  if (lane == 0) { s_best[wave] = best; s_bidx[wave] = best_j; s_binv[wave] = best_inv; }
  __syncthreads();
  int w = 0;
  for (int c = 1; c < 4; ++c)
    if (s_best[c] > s_best[w] || (s_best[c] == s_best[w] && s_bidx[c] < s_bidx[w])) w = c;
  int nn = s_bidx[w];
  float inv_nn = s_binv[w];
  if (nn >= n) { nn = i == 0 ? 1 : 0; inv_nn = 0.f; }  // no candidate compared greater (NaN rows): a valid index, a NaN distance
  const T* xn = x + (size_t)nn * ldx;
  float dd = 0.f;
  for (int k = threadIdx.x * 4; k < D; k += 1024) {
    const f32x4 v = Vec4<T>::load(xn + k) * inv_nn, a = *reinterpret_cast<const f32x4*>(s_xi + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float u = a[e] - v[e] + kKoleoEps;
      dd += u * u;
    }
  }
  dd = block_sum4(dd, s_red);
  if (threadIdx.x == 0) {
    nn_index[i] = nn;
    dist[i] = sqrtf(dd);
    inv_norm[i] = inv_i;
  }
}

// loss = - mean_i log(dist_i + eps), rows in a fixed order
__global__ void __launch_bounds__(256) koleo_loss_kernel(const float* __restrict__ dist, int n, float* __restrict__ loss) {
  __shared__ float s_red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += logf(dist[i] + kKoleoEps);
  s = block_sum4(s, s_red);
  if (threadIdx.x == 0) *loss = -s / (float)n;
}

// one block per row i; dynamic LDS: 2 D floats (xh_i, dxh_i)
template <typename T>
__global__ void __launch_bounds__(256) koleo_bwd_kernel(const T* __restrict__ x, int n, int D, int64_t ldx, const int32_t* __restrict__ nn_index,
                                                        const float* __restrict__ dist, const float* __restrict__ inv_norm,
                                                        const float* __restrict__ dloss, T* __restrict__ dx, int64_t lddx) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  __shared__ float s_red[4];
  float* s_xi = s_mem;
  float* s_g = s_mem + D;
  const int i = blockIdx.x;
  const float g = -(dloss ? *dloss : 1.0f) / (float)n;
  const T* xi = x + (size_t)i * ldx;
  const float inv_i = inv_norm[i];
  // own term: G_i = c_i (xh_i - xh_I + eps)
  {
    const int nn = min(max(nn_index[i], 0), n - 1);
    const float di = dist[i], ci = g / ((di + kKoleoEps) * di), inv_nn = inv_norm[nn];
    const T* xn = x + (size_t)nn * ldx;
    for (int k = threadIdx.x * 4; k < D; k += 1024) {
      const f32x4 a = Vec4<T>::load(xi + k) * inv_i, v = Vec4<T>::load(xn + k) * inv_nn;
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = ci * (a[e] - v[e] + kKoleoEps);
      *reinterpret_cast<f32x4*>(s_xi + k) = a;
      *reinterpret_cast<f32x4*>(s_g + k) = o;
    }
  }
  // the rows that chose i, in row order: - G_j = - c_j (xh_j - xh_i + eps).  (each thread touches only its own k: no barrier needed)
  for (int j = 0; j < n; ++j) {
    if (nn_index[j] != i) continue;
    const float dj = dist[j], cj = g / ((dj + kKoleoEps) * dj), inv_j = inv_norm[j];
    const T* xj = x + (size_t)j * ldx;
    for (int k = threadIdx.x * 4; k < D; k += 1024) {
      const f32x4 v = Vec4<T>::load(xj + k) * inv_j, a = *reinterpret_cast<const f32x4*>(s_xi + k);
      f32x4 o = *reinterpret_cast<const f32x4*>(s_g + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] -= cj * (v[e] - a[e] + kKoleoEps);
      *reinterpret_cast<f32x4*>(s_g + k) = o;
    }
  }
  float p = 0.f;
  for (int k = threadIdx.x * 4; k < D; k += 1024) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(s_xi + k), o = *reinterpret_cast<const f32x4*>(s_g + k);
    p += (a[0] * o[0] + a[1] * o[1]) + (a[2] * o[2] + a[3] * o[3]);
  }
  p = block_sum4(p, s_red);
  T* out = dx + (size_t)i * lddx;
  for (int k = threadIdx.x * 4; k < D; k += 1024) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(s_xi + k), o = *reinterpret_cast<const f32x4*>(s_g + k);
    Vec4<T>::store(out + k, (o - a * p) * inv_i);
  }
}

constexpr int kKoleoMaxD = 4096;  // 2 D floats of LDS in the backward: 32 KiB

}  // namespace
}  // namespace hct

using namespace hct;

extern "C" {

int hct_koleo_fwd(const void* x, int dtype, int n, int D, int64_t ldx, float* loss, int32_t* nn_index, float* dist, float* inv_norm, void* stream) {
  HCT_REQUIRE(x && loss && nn_index && dist && inv_norm, "hct_koleo_fwd: null buffer");
  HCT_REQUIRE(dtype == HCT_F32 || dtype == HCT_BF16, "hct_koleo_fwd: rows must be fp32 or bf16");
  HCT_REQUIRE(n >= 2 && D > 0 && D % 4 == 0 && D <= kKoleoMaxD && ldx >= D && ldx % 4 == 0,
              "hct_koleo_fwd: needs n >= 2 rows, D %% 4 == 0, D <= 4096 and a row stride >= D that is a multiple of 4");
  HCT_REQUIRE((uintptr_t)x % (4 * dtype_size(dtype)) == 0, "hct_koleo_fwd: rows must be aligned to 4 elements");
  hipStream_t s = (hipStream_t)stream;
  HCT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(koleo_fwd_kernel<T>, dim3(n), dim3(256), (size_t)D * sizeof(float), s, (const T*)x, n, D, ldx, nn_index,
                                                   dist, inv_norm));
  hipLaunchKernelGGL(koleo_loss_kernel, dim3(1), dim3(256), 0, s, dist, n, loss);
  HCT_CHECK_LAUNCH("hct_koleo_fwd");
  return 0;
}

int hct_koleo_bwd(const void* x, int dtype, int n, int D, int64_t ldx, const int32_t* nn_index, const float* dist, const float* inv_norm,
                  const float* dloss, void* dx, int64_t lddx, void* stream) {
  HCT_REQUIRE(x && nn_index && dist && inv_norm && dx, "hct_koleo_bwd: null buffer");
  HCT_REQUIRE(dtype == HCT_F32 || dtype == HCT_BF16, "hct_koleo_bwd: rows must be fp32 or bf16");
  HCT_REQUIRE(n >= 2 && D > 0 && D % 4 == 0 && D <= kKoleoMaxD && ldx >= D && ldx % 4 == 0 && lddx >= D && lddx % 4 == 0,
              "hct_koleo_bwd: needs n >= 2 rows, D %% 4 == 0, D <= 4096 and row strides >= D that are multiples of 4");
  HCT_REQUIRE((uintptr_t)x % (4 * dtype_size(dtype)) == 0 && (uintptr_t)dx % (4 * dtype_size(dtype)) == 0, "hct_koleo_bwd: rows must be aligned to 4 elements");
  HCT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(koleo_bwd_kernel<T>, dim3(n), dim3(256), (size_t)2 * D * sizeof(float), (hipStream_t)stream, (const T*)x, n,
                                                   D, ldx, nn_index, dist, inv_norm, dloss, (T*)dx, lddx));
  HCT_CHECK_LAUNCH("hct_koleo_bwd");
  return 0;
}

}  // extern "C"
