// Segmentation fine-tuning: Dice + cross-entropy over the voxels of a batch, read from the decoder's logits in TOKEN layout
// (hct_seg_loss), the arg-max prediction with its confusion counts (hct_seg_predict) and the label twin of the pool gather
// (hct_gather_flip_labels), and a mask file's voxels as the label item of the image's cache item (hct_label_to_item).  An addition of this build: the reference has no per-voxel task.
//
// Layout.  The linear decoder gives one row of K * P^3 logits per token; column c * P^3 + v is class c at voxel
// v = (pz * P + py) * P + px of the patch, patch l = (lz * G + ly) * G + lx of sample b is row b * T + first + l, and the voxel lies
// at z = lz * P + pz (likewise y, x) of the label volume [B, S, S, S], S = G * P.  The logits are never un-patchified: an item is
// V consecutive voxels along v (V = 4 when P, the row strides and the pointers allow 4-wide access, else 1), which are V
// consecutive px of one label row and, per class, V consecutive columns of one logits row.
//
// Work split, the same for every kernel here: a sample has S^3 / V items; a block of 256 threads takes `trips` rounds of 256
// consecutive items (thread tid takes item base + t * 256 + tid), trips chosen so that a sample has at most 64 blocks.
// grid = (blocks per sample, B).  Everything a block sums leaves it as ONE partial per quantity: lanes by the xor butterfly,
// the four waves in index order.  No atomics anywhere; a repeated call is bit-identical.
//
// hct_seg_loss, three phases on the caller's stream:
//   stats     per valid voxel the softmax in fp32 (row maximum subtracted, expf, one division), then per block the partials
//             (sum w_y * nll, sum w_y, I_c, P_c, Y_c) -> workspace.
//   finalize  one block, double: per (b, c) the block partials in index order, dice_bc, the gradient's coefficients
//             alpha_bc, beta_bc (dDice/dp_c = alpha_bc [y = c] + beta_bc, w_dice folded in); per b the CE sums; then a halving tree
//             over the 256 threads.
//   gradient  the thread that reads a voxel's K logits writes its K gradients, so dlogits may be the logits buffer itself.
//             Ignored voxels get zeros; a second small launch zeroes the `first` leading rows of every sample.
#include "common.h"
#include "prof.h"

#include <algorithm>

namespace hct {
namespace {

constexpr int kSegThreads = 256;
constexpr int kSegMaxK = 16;
constexpr int kSegMaxBlocks = 64;  // blocks (= partials) per sample
constexpr size_t kSegHead = 16;    // workspace head: the CE scale w_ce / sum w (float), padded
constexpr double kSegEps = 1e-5;   // MONAI DiceLoss smooth_nr = smooth_dr

struct SegShape {
  int vec, items, trips, nb;
};

SegShape seg_shape(int S, int vec) {
  SegShape s;
  s.vec = vec;
  s.items = S * S * S / vec;
  const int rounds = (s.items + kSegThreads - 1) / kSegThreads;
  s.trips = (rounds + kSegMaxBlocks - 1) / kSegMaxBlocks;
  s.nb = (rounds + s.trips - 1) / s.trips;
  return s;
}

template <typename T, int V> __device__ __forceinline__ void seg_load(const T* p, float (&x)[V]) {
  if constexpr (V == 4) {
    const f32x4 v = Vec4<T>::load(p);
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = v[q];
  } else {
    x[0] = to_f32(p[0]);
  }
}
template <typename T, int V> __device__ __forceinline__ void seg_store(T* p, const float (&x)[V]) {
  if constexpr (V == 4) {
    Vec4<T>::store(p, f32x4{x[0], x[1], x[2], x[3]});
  } else {
    p[0] = from_f32<T>(x[0]);
  }
}
template <int V> __device__ __forceinline__ void seg_load_labels(const uint8_t* p, int (&y)[V]) {
  if constexpr (V == 4) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int q = 0; q < 4; ++q) y[q] = (int)((w >> (8 * q)) & 255u);
  } else {
    y[0] = p[0];
  }
}

// where item `it` of sample b lies: the element offset of its first logit (class 0) and of its first label
struct SegGeom {
  int T, first, G, P, S, P3, ipp;  // ipp: items per patch
  __device__ __forceinline__ void locate(int b, int it, int V, int64_t ld, int64_t& xoff, int64_t& yoff) const {
    const int l = it / ipp, v = (it - l * ipp) * V;
    const int px = v % P, r = v / P, py = r % P, pz = r / P;
    const int lx = l % G, q = l / G, ly = q % G, lz = q / G;
    xoff = ((int64_t)b * T + first + l) * ld + v;
    yoff = (((int64_t)b * S + lz * P + pz) * S + ly * P + py) * S + lx * P + px;
  }
};

// softmax of one voxel in place: x_k -> p_k; returns log(sum exp(x - max)) and leaves the maximum in m
template <int KT> __device__ __forceinline__ float seg_softmax(float (&x)[KT], int K, float& m) {
  m = x[0];
#pragma unroll
  for (int k = 1; k < KT; ++k)
    if (k < K) m = fmaxf(m, x[k]);
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < KT; ++k)
    if (k < K) {
      x[k] = expf(x[k] - m);
      s += x[k];
    }
  const float inv = 1.0f / s;
#pragma unroll
  for (int k = 0; k < KT; ++k)
    if (k < K) x[k] *= inv;
  return logf(s);
}

// the nq per-thread sums of a block -> out[q]: xor butterfly over the lanes, then the four waves in index order
template <int NQ> __device__ __forceinline__ void seg_block_sums(float (&acc)[NQ], int nq, float* __restrict__ out) {
  __shared__ float lds[kSegThreads / kWave][NQ];
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (q < nq) {
      const float v = wave_sum(acc[q]);
      if (lane == 0) lds[wave][q] = v;
    }
  __syncthreads();
  if (tid < nq) {
    float v = lds[0][tid];
    for (int w = 1; w < kSegThreads / kWave; ++w) v += lds[w][tid];
    out[tid] = v;
  }
}

template <typename T, int V, int KT>
__global__ void __launch_bounds__(kSegThreads) seg_stats_kernel(const T* __restrict__ logits, int64_t ld, const uint8_t* __restrict__ labels,
                                                                const float* __restrict__ class_weight, SegGeom g, int K, int items,
                                                                int trips, float* __restrict__ partial) {
  // acc: [0] sum w_y nll, [1] sum w_y, [2 + c] I_c, [2 + KT + c] P_c, [2 + 2 KT + c] Y_c
  float acc[2 + 3 * KT];
#pragma unroll
  for (int q = 0; q < 2 + 3 * KT; ++q) acc[q] = 0.0f;
  float cw[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) cw[k] = (class_weight && k < K) ? class_weight[k] : 1.0f;
  const int b = blockIdx.y;
  const int base = blockIdx.x * trips * kSegThreads + threadIdx.x;
  for (int t = 0; t < trips; ++t) {
    const int it = base + t * kSegThreads;
    if (it >= items) break;
    int64_t xoff, yoff;
    g.locate(b, it, V, ld, xoff, yoff);
    int y[V];
    seg_load_labels<V>(labels + yoff, y);
    float x[KT][V];
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) seg_load<T, V>(logits + xoff + (int64_t)k * g.P3, x[k]);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      if (y[q] >= K) continue;  // 255 = ignore (and anything else that names no class)
      float p[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) p[k] = k < K ? x[k][q] : 0.0f;
      float xy = 0.0f, wy = 0.0f, m;
#pragma unroll
      for (int k = 0; k < KT; ++k)
        if (k < K && y[q] == k) {
          xy = p[k];
          wy = cw[k];
        }
      const float lse = seg_softmax<KT>(p, K, m);
      acc[0] += wy * (lse - (xy - m));
      acc[1] += wy;
#pragma unroll
      for (int k = 0; k < KT; ++k)
        if (k < K) {
          const float hit = y[q] == k ? 1.0f : 0.0f;
          acc[2 + k] += p[k] * hit;
          acc[2 + KT + k] += p[k];
          acc[2 + 2 * KT + k] += hit;
        }
    }
  }
  // partial row = [ce, w, I[KT], P[KT], Y[KT]]: the class arrays keep the compiled bound KT as their stride
  constexpr int nq = 2 + 3 * KT;
  seg_block_sums<nq>(acc, nq, partial + ((size_t)b * gridDim.x + blockIdx.x) * nq);
}

__global__ void __launch_bounds__(kSegThreads) seg_finalize_kernel(const float* __restrict__ partial, int B, int K, int kt, int nb,
                                                                   float w_ce, float w_dice, float* __restrict__ loss, float* __restrict__ ce,
                                                                   float* __restrict__ dice, float* __restrict__ dice_bc,
                                                                   float* __restrict__ coef, float* __restrict__ head) {
  __shared__ double sd[kSegThreads], sc[kSegThreads], sw[kSegThreads];
  const int tid = threadIdx.x, nq = 2 + 3 * kt;  // kt: the class stride of a partial row
  const double bk = (double)B * (double)K;
  double accd = 0.0, accc = 0.0, accw = 0.0;
  for (int pair = tid; pair < B * K; pair += kSegThreads) {
    const int b = pair / K, c = pair - b * K;
    double I = 0.0, Pc = 0.0, Y = 0.0;
    for (int j = 0; j < nb; ++j) {
      const float* p = partial + ((size_t)b * nb + j) * nq;
      I += (double)p[2 + c];
      Pc += (double)p[2 + kt + c];
      Y += (double)p[2 + 2 * kt + c];
    }
    const double num = 2.0 * I + kSegEps, den = Pc + Y + kSegEps, d = num / den;
    if (dice_bc) dice_bc[pair] = (float)d;
    accd += 1.0 - d;
    coef[2 * pair] = (float)((double)w_dice * (-2.0 / (bk * den)));
    coef[2 * pair + 1] = (float)((double)w_dice * (num / (bk * den * den)));
  }
  for (int b = tid; b < B; b += kSegThreads)
    for (int j = 0; j < nb; ++j) {
      const float* p = partial + ((size_t)b * nb + j) * nq;
      accc += (double)p[0];
      accw += (double)p[1];
    }
  sd[tid] = accd;
  sc[tid] = accc;
  sw[tid] = accw;
  __syncthreads();
  for (int o = kSegThreads >> 1; o > 0; o >>= 1) {
    if (tid < o) {
      sd[tid] += sd[tid + o];
      sc[tid] += sc[tid + o];
      sw[tid] += sw[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double w = sw[0];
    const double vce = w > 0.0 ? sc[0] / w : 0.0, vdice = sd[0] / bk;
    if (ce) ce[0] = (float)vce;
    if (dice) dice[0] = (float)vdice;
    if (loss) loss[0] = (float)((double)w_ce * vce + (double)w_dice * vdice);
    head[0] = w > 0.0 ? (float)((double)w_ce / w) : 0.0f;
  }
}

// logits and dlogits may be the same buffer: no __restrict__ on either, and a thread has read its K * V logits before it stores
template <typename T, int V, int KT>
__global__ void __launch_bounds__(kSegThreads) seg_grad_kernel(const T* logits, int64_t ld, const uint8_t* __restrict__ labels,
                                                               const float* __restrict__ class_weight, SegGeom g, int K, int items,
                                                               int trips, const float* __restrict__ coef, const float* __restrict__ head,
                                                               const float* __restrict__ dloss, T* dlogits, int64_t ldd) {
  const int b = blockIdx.y;
  float al[KT], be[KT], cw[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    al[k] = k < K ? coef[2 * ((size_t)b * K + k)] : 0.0f;
    be[k] = k < K ? coef[2 * ((size_t)b * K + k) + 1] : 0.0f;
    cw[k] = (class_weight && k < K) ? class_weight[k] : 1.0f;
  }
  const float ces = head[0], gl = dloss ? dloss[0] : 1.0f;
  const int base = blockIdx.x * trips * kSegThreads + threadIdx.x;
  for (int t = 0; t < trips; ++t) {
    const int it = base + t * kSegThreads;
    if (it >= items) break;
    int64_t xoff, yoff;
    g.locate(b, it, V, ld, xoff, yoff);
    const int64_t doff = xoff + (((int64_t)b * g.T + g.first + it / g.ipp)) * (ldd - ld);
    int y[V];
    seg_load_labels<V>(labels + yoff, y);
    float x[KT][V];
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) seg_load<T, V>(logits + xoff + (int64_t)k * g.P3, x[k]);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      float p[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) p[k] = k < K ? x[k][q] : 0.0f;
      if (y[q] >= K) {
#pragma unroll
        for (int k = 0; k < KT; ++k) x[k][q] = 0.0f;
        continue;
      }
      float m, wy = 0.0f;
      seg_softmax<KT>(p, K, m);
      float gk[KT], dot = 0.0f;
#pragma unroll
      for (int k = 0; k < KT; ++k)
        if (k < K) {
          const bool hit = y[q] == k;
          if (hit) wy = cw[k];
          gk[k] = hit ? al[k] + be[k] : be[k];
          dot += gk[k] * p[k];
        }
      const float cs = wy * ces;
#pragma unroll
      for (int k = 0; k < KT; ++k)
        if (k < K) {
          const float hit = y[q] == k ? 1.0f : 0.0f;
          // the loss's own gradient first, dloss last: a power-of-two dloss scales every bit pattern exactly
          x[k][q] = (p[k] * (gk[k] - dot) + cs * (p[k] - hit)) * gl;
        }
    }
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) seg_store<T, V>(dlogits + doff + (int64_t)k * g.P3, x[k]);
  }
}

// zeros in the `first` leading rows (class token, registers) of every sample: cols = K * P^3 columns of row b * T + r
template <typename T, int V>
__global__ void __launch_bounds__(kSegThreads) seg_zero_rows_kernel(T* __restrict__ d, int64_t ldd, int B, int T_, int first, int cols) {
  const int cv = cols / V;
  const int64_t total = (int64_t)B * first * cv;
  const float z[V] = {};
  for (int64_t e = (int64_t)blockIdx.x * kSegThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kSegThreads) {
    const int c = (int)(e % cv);
    const int64_t r = e / cv;
    const int64_t row = (r / first) * T_ + (r % first);
    seg_store<T, V>(d + row * ldd + (int64_t)c * V, z);
  }
}

// ---- prediction --------------------------------------------------------------------------------------------------------------
template <typename T, int V, int KT>
__global__ void __launch_bounds__(kSegThreads) seg_predict_kernel(const T* __restrict__ logits, int64_t ld, const uint8_t* __restrict__ labels,
                                                                  SegGeom g, int K, int items, int trips, int prob_class,
                                                                  uint8_t* __restrict__ pred, f16* __restrict__ prob,
                                                                  int* __restrict__ partial) {
  __shared__ int lds[kSegThreads / kWave][3 * KT];
  int cnt[3 * KT];  // [3 k + 0 / 1 / 2] = TP / FP / FN of class k
#pragma unroll
  for (int q = 0; q < 3 * KT; ++q) cnt[q] = 0;
  const int b = blockIdx.y;
  const int base = blockIdx.x * trips * kSegThreads + threadIdx.x;
  for (int t = 0; t < trips; ++t) {
    const int it = base + t * kSegThreads;
    if (it >= items) break;
    int64_t xoff, yoff;
    g.locate(b, it, V, ld, xoff, yoff);
    int y[V];
    if (labels) seg_load_labels<V>(labels + yoff, y);
    float x[KT][V];
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) seg_load<T, V>(logits + xoff + (int64_t)k * g.P3, x[k]);
    int a[V];
    float pr[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      float m = x[0][q];
      a[q] = 0;
#pragma unroll
      for (int k = 1; k < KT; ++k)
        if (k < K && x[k][q] > m) {  // strictly greater: ties stay with the lowest class
          m = x[k][q];
          a[q] = k;
        }
      if (prob) {
        float s = 0.0f, e = 0.0f;
#pragma unroll
        for (int k = 0; k < KT; ++k)
          if (k < K) {
            const float v = expf(x[k][q] - m);
            s += v;
            if (k == prob_class) e = v;
          }
        pr[q] = e / s;
      }
      if (labels && y[q] < K) {
#pragma unroll
        for (int k = 0; k < KT; ++k)
          if (k < K) {
            const bool isa = a[q] == k, isy = y[q] == k;
            cnt[3 * k] += (isa && isy) ? 1 : 0;
            cnt[3 * k + 1] += (isa && !isy) ? 1 : 0;
            cnt[3 * k + 2] += (!isa && isy) ? 1 : 0;
          }
      }
    }
    if (pred) {
      if constexpr (V == 4) {
        const uint32_t w = (uint32_t)a[0] | ((uint32_t)a[1] << 8) | ((uint32_t)a[2] << 16) | ((uint32_t)a[3] << 24);
        *reinterpret_cast<uint32_t*>(pred + yoff) = w;
      } else {
        pred[yoff] = (uint8_t)a[0];
      }
    }
    if (prob) {
      if constexpr (V == 4) {
        const f16x4 h = {(f16)pr[0], (f16)pr[1], (f16)pr[2], (f16)pr[3]};
        *reinterpret_cast<f16x4*>(prob + yoff) = h;
      } else {
        prob[yoff] = (f16)pr[0];
      }
    }
  }
  if (!partial) return;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
#pragma unroll
  for (int q = 0; q < 3 * KT; ++q)
    if (q < 3 * K) {
      int v = cnt[q];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) lds[wave][q] = v;
    }
  __syncthreads();
  if (tid < 3 * K) {
    int v = 0;
    for (int w = 0; w < kSegThreads / kWave; ++w) v += lds[w][tid];
    partial[((size_t)b * gridDim.x + blockIdx.x) * 3 * K + tid] = v;
  }
}

__global__ void __launch_bounds__(kSegThreads) seg_counts_kernel(const int* __restrict__ partial, int B, int K, int nb, long long* __restrict__ counts) {
  const int n = B * K * 3;
  for (int e = blockIdx.x * kSegThreads + threadIdx.x; e < n; e += gridDim.x * kSegThreads) {
    const int b = e / (3 * K), q = e - b * 3 * K;
    long long v = 0;
    for (int j = 0; j < nb; ++j) v += partial[((size_t)b * nb + j) * 3 * K + q];
    counts[e] = v;
  }
}

// ---- labels out of a stacked pool, flipped -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSegThreads) gather_flip_labels_kernel(const uint8_t* __restrict__ pool, const int32_t* __restrict__ slot,
                                                                         uint8_t* __restrict__ out, int S, int64_t n_slots,
                                                                         const unsigned char* __restrict__ flip, int per_vol) {
  const int b = blockIdx.y;
  const int64_t sl = slot[b];
  const bool none = sl < 0 || sl >= n_slots;  // -1 by contract; anything else outside the pool is never dereferenced either
  const unsigned f = flip ? flip[b] : 0u;
  const int64_t vol = (int64_t)S * S * S;
  const uint8_t* src = pool + (none ? 0 : sl) * vol;
  uint8_t* dst = out + (int64_t)b * vol;
  const int sv = S / 4;
  const bool rev = (f & 4u) != 0;
  for (int u = blockIdx.x * kSegThreads + threadIdx.x; u < per_vol; u += gridDim.x * kSegThreads) {
    const int kv = u % sv, r = u / sv;
    const int j = r % S, i = r / S;
    const int si = (f & 1u) ? S - 1 - i : i, sj = (f & 2u) ? S - 1 - j : j;
    const int sk = rev ? S - 4 - kv * 4 : kv * 4;
    uint32_t w = 0xffffffffu;
    if (!none) {
      w = *reinterpret_cast<const uint32_t*>(src + ((int64_t)si * S + sj) * S + sk);
      if (rev) w = __builtin_bswap32(w);
    }
    *reinterpret_cast<uint32_t*>(dst + ((int64_t)i * S + j) * S + kv * 4) = w;
  }
}

int seg_kt(int K) { return K <= 4 ? std::max(K, 2) : K <= 6 ? 6 : K <= 8 ? 8 : kSegMaxK; }  // HCT_SEG_DISPATCH_K's choice

// ---- label item: nearest neighbour through the image's geometry -------------------------------------------------------------------
// one thread per output voxel; the box is read from the device words the image's loading chain left (confined to the volume
// here), the cell centre of the resize is taken in integers, the spacing step is the host's table `near`
__global__ void __launch_bounds__(kSegThreads) label_to_item_kernel(const float* __restrict__ ras, int d0, int d1, int d2,
                                                                    const int32_t* __restrict__ near, int m0, int m1, int m2,
                                                                    const int32_t* __restrict__ box, uint8_t* __restrict__ out, int R0, int R1,
                                                                    int R2, int32_t* __restrict__ status) {
  const int64_t total = (int64_t)R0 * R1 * R2;
  const int d[3] = {d0, d1, d2}, m[3] = {m0, m1, m2}, R[3] = {R0, R1, R2};
  int start[3], size[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    start[a] = min(max(box[a], 0), m[a] - 1);
    size[a] = min(max(box[3 + a], 1), m[a] - start[a]);
  }
  const int32_t* tab[3] = {near, near + m0, near + m0 + m1};
  for (int64_t e = (int64_t)blockIdx.x * kSegThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kSegThreads) {
    const int o[3] = {(int)(e / ((int64_t)R1 * R2)), (int)((e / R2) % R1), (int)(e % R2)};
    int r[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int64_t cell = ((int64_t)(2 * o[a] + 1) * size[a]) / (2 * (int64_t)R[a]);
      const int c = start[a] + (int)min<int64_t>(size[a] - 1, cell);
      r[a] = min(max(tab[a][c], 0), d[a] - 1);
    }
    const float v = ras[((int64_t)r[0] * d1 + r[1]) * d2 + r[2]];
    const bool good = v >= 0.0f && v <= 254.0f && v == floorf(v);
    if (!good) status[0] = HCT_LABEL_BAD_VALUE;  // every offender stores the same word
    out[e] = good ? (uint8_t)v : (uint8_t)255;
  }
}

bool seg_aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

int seg_check_shape(const char* what, int B, int T, int first, int G, int P, int K, int64_t ld) {
  HCT_REQUIRE(B >= 1 && B <= 65535 && G >= 1 && P >= 1 && K >= 2 && K <= kSegMaxK && first >= 0,
              "%s: bad shape (B %d in [1, 65535], G %d, P %d, K %d in [2, %d], first %d)", what, B, G, P, K, kSegMaxK, first);
  HCT_REQUIRE((int64_t)G * P <= 1024, "%s: volume side G * P = %lld above 1024", what, (long long)G * P);
  HCT_REQUIRE((int64_t)T >= (int64_t)first + (int64_t)G * G * G, "%s: T %d < first %d + G^3 %lld", what, T, first, (long long)G * G * G);
  HCT_REQUIRE(ld >= (int64_t)K * P * P * P, "%s: row stride %lld < K * P^3 = %lld", what, (long long)ld, (long long)K * P * P * P);
  return 0;
}

}  // namespace
}  // namespace hct

using namespace hct;

// K -> the smallest compiled class bound that holds it
#define HCT_SEG_DISPATCH_K(K, ...)          \
  do {                                      \
    if ((K) <= 2) {                         \
      constexpr int KT = 2;                 \
      __VA_ARGS__;                          \
    } else if ((K) <= 3) {                  \
      constexpr int KT = 3;                 \
      __VA_ARGS__;                          \
    } else if ((K) <= 4) {                  \
      constexpr int KT = 4;                 \
      __VA_ARGS__;                          \
    } else if ((K) <= 6) {                  \
      constexpr int KT = 6;                 \
      __VA_ARGS__;                          \
    } else if ((K) <= 8) {                  \
      constexpr int KT = 8;                 \
      __VA_ARGS__;                          \
    } else {                                \
      constexpr int KT = kSegMaxK;          \
      __VA_ARGS__;                          \
    }                                       \
  } while (0)
#define HCT_SEG_DISPATCH_V(vec, ...) \
  do {                               \
    if ((vec) == 4) {                \
      constexpr int V = 4;           \
      __VA_ARGS__;                   \
    } else {                         \
      constexpr int V = 1;           \
      __VA_ARGS__;                   \
    }                                \
  } while (0)

extern "C" {

size_t hct_seg_loss_workspace_bytes(int B, int G, int P, int K) {
  if (B < 1 || G < 1 || P < 1 || K < 2 || K > kSegMaxK || (int64_t)G * P > 1024) return 0;
  // sized for one-voxel items (the most blocks per sample the entry point can choose)
  const SegShape sh = seg_shape(G * P, 1);
  return kSegHead + (size_t)B * K * 2 * sizeof(float) + (size_t)B * sh.nb * (2 + 3 * seg_kt(K)) * sizeof(float);
}

int hct_seg_loss(const void* logits, int dtype, int64_t ld, const uint8_t* labels, const float* class_weight, int B, int T, int first, int G,
                 int P, int K, float w_ce, float w_dice, const float* dloss, float* loss, float* ce, float* dice, float* dice_bc,
                 void* dlogits, int64_t ldd, int reuse_stats, void* workspace, size_t workspace_bytes, void* stream) {
  HCT_REQUIRE(logits && labels && (dtype == HCT_F32 || dtype == HCT_BF16), "hct_seg_loss: null logits / labels or a dtype that is neither fp32 nor bf16");
  if (int rc = seg_check_shape("hct_seg_loss", B, T, first, G, P, K, ld)) return rc;
  HCT_REQUIRE(loss || ce || dice || dice_bc || dlogits, "hct_seg_loss: nothing to compute (no output given)");
  HCT_REQUIRE(!dlogits || ldd >= (int64_t)K * P * P * P, "hct_seg_loss: dlogits row stride %lld < K * P^3", (long long)ldd);
  HCT_REQUIRE(!reuse_stats || (dlogits && !loss && !ce && !dice && !dice_bc),
              "hct_seg_loss: reuse_stats runs the gradient phase alone (dlogits, no loss outputs)");
  const size_t need = hct_seg_loss_workspace_bytes(B, G, P, K);
  if (!workspace || workspace_bytes < need || !seg_aligned(workspace, 16)) {
    set_error("hct_seg_loss: workspace too small or not 16-byte aligned (%zu < %zu)", workspace_bytes, need);
    return HCT_E_WORKSPACE;
  }
  const size_t es = dtype_size(dtype);
  const int S = G * P, P3 = P * P * P;
  const bool wide = P % 4 == 0 && ld % 4 == 0 && seg_aligned(logits, 4 * es) && seg_aligned(labels, 4) &&
                    (!dlogits || (ldd % 4 == 0 && seg_aligned(dlogits, 4 * es)));
  const SegShape sh = seg_shape(S, wide ? 4 : 1);
  const SegGeom g = {T, first, G, P, S, P3, P3 / sh.vec};
  float* head = (float*)workspace;
  float* coef = (float*)((char*)workspace + kSegHead);
  float* partial = coef + (size_t)B * K * 2;
  hipStream_t s = (hipStream_t)stream;
  const double voxels = (double)B * S * S * S, lbytes = voxels * K * (double)es;
  ProfScope ps(PROF_SEG, voxels, s, (reuse_stats ? 0.0 : lbytes + voxels) + (dlogits ? 2.0 * lbytes + voxels : 0.0));
  const dim3 grid(sh.nb, B), block(kSegThreads);
  if (!reuse_stats) {
    HCT_DISPATCH_DTYPE(dtype, Tt, HCT_SEG_DISPATCH_V(sh.vec, HCT_SEG_DISPATCH_K(K,
        hipLaunchKernelGGL((seg_stats_kernel<Tt, V, KT>), grid, block, 0, s, (const Tt*)logits, ld, labels, class_weight, g, K, sh.items,
                           sh.trips, partial))));
    hipLaunchKernelGGL(seg_finalize_kernel, dim3(1), block, 0, s, partial, B, K, seg_kt(K), sh.nb, w_ce, w_dice, loss, ce, dice, dice_bc, coef, head);
  }
  if (dlogits) {
    HCT_DISPATCH_DTYPE(dtype, Tt, HCT_SEG_DISPATCH_V(sh.vec, HCT_SEG_DISPATCH_K(K,
        hipLaunchKernelGGL((seg_grad_kernel<Tt, V, KT>), grid, block, 0, s, (const Tt*)logits, ld, labels, class_weight, g, K, sh.items,
                           sh.trips, coef, head, dloss, (Tt*)dlogits, ldd))));
    if (first > 0) {
      const int cols = K * P3;
      const int64_t total = (int64_t)B * first * (cols / sh.vec);
      const int zgrid = (int)std::min<int64_t>(1024, (total + kSegThreads - 1) / kSegThreads);
      HCT_DISPATCH_DTYPE(dtype, Tt, HCT_SEG_DISPATCH_V(sh.vec,
          hipLaunchKernelGGL((seg_zero_rows_kernel<Tt, V>), dim3(zgrid), block, 0, s, (Tt*)dlogits, ldd, B, T, first, cols)));
    }
  }
  HCT_CHECK_LAUNCH("hct_seg_loss");
  return 0;
}

size_t hct_seg_predict_workspace_bytes(int B, int G, int P, int K) {
  if (B < 1 || G < 1 || P < 1 || K < 2 || K > kSegMaxK || (int64_t)G * P > 1024) return 0;
  const SegShape sh = seg_shape(G * P, 1);
  return (size_t)B * sh.nb * 3 * K * sizeof(int);
}

int hct_seg_predict(const void* logits, int dtype, int64_t ld, const uint8_t* labels, int B, int T, int first, int G, int P, int K,
                    int prob_class, uint8_t* pred, void* prob, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  HCT_REQUIRE(logits && (dtype == HCT_F32 || dtype == HCT_BF16), "hct_seg_predict: null logits or a dtype that is neither fp32 nor bf16");
  if (int rc = seg_check_shape("hct_seg_predict", B, T, first, G, P, K, ld)) return rc;
  HCT_REQUIRE(pred || prob || counts, "hct_seg_predict: nothing to compute (no output given)");
  HCT_REQUIRE(!counts || labels, "hct_seg_predict: counts need labels");
  HCT_REQUIRE(!prob || (prob_class >= 0 && prob_class < K), "hct_seg_predict: prob_class %d outside [0, %d)", prob_class, K);
  if (counts) {
    const size_t need = hct_seg_predict_workspace_bytes(B, G, P, K);
    if (!workspace || workspace_bytes < need || !seg_aligned(workspace, 4)) {
      set_error("hct_seg_predict: workspace too small or not 4-byte aligned (%zu < %zu)", workspace_bytes, need);
      return HCT_E_WORKSPACE;
    }
  }
  const size_t es = dtype_size(dtype);
  const int S = G * P, P3 = P * P * P;
  const bool wide = P % 4 == 0 && ld % 4 == 0 && seg_aligned(logits, 4 * es) && (!labels || seg_aligned(labels, 4)) &&
                    (!pred || seg_aligned(pred, 4)) && (!prob || seg_aligned(prob, 8));
  const SegShape sh = seg_shape(S, wide ? 4 : 1);
  const SegGeom g = {T, first, G, P, S, P3, P3 / sh.vec};
  hipStream_t s = (hipStream_t)stream;
  const double voxels = (double)B * S * S * S;
  ProfScope ps(PROF_SEG, voxels, s, voxels * K * (double)es + voxels * ((labels ? 1.0 : 0.0) + (pred ? 1.0 : 0.0) + (prob ? 2.0 : 0.0)));
  const dim3 grid(sh.nb, B), block(kSegThreads);
  const uint8_t* lab = counts ? labels : nullptr;
  int* partial = counts ? (int*)workspace : nullptr;
  HCT_DISPATCH_DTYPE(dtype, Tt, HCT_SEG_DISPATCH_V(sh.vec, HCT_SEG_DISPATCH_K(K,
      hipLaunchKernelGGL((seg_predict_kernel<Tt, V, KT>), grid, block, 0, s, (const Tt*)logits, ld, lab, g, K, sh.items, sh.trips, prob_class,
                         pred, (f16*)prob, partial))));
  if (counts) {
    const int n = B * K * 3;
    hipLaunchKernelGGL(seg_counts_kernel, dim3(std::min(256, (n + kSegThreads - 1) / kSegThreads)), block, 0, s, partial, B, K, sh.nb,
                       (long long*)counts);
  }
  HCT_CHECK_LAUNCH("hct_seg_predict");
  return 0;
}

int hct_gather_flip_labels(const uint8_t* pool, const int32_t* slot, uint8_t* out, int B, int S, int64_t n_slots, const unsigned char* flip,
                           void* stream) {
  HCT_REQUIRE(pool && slot && out && B > 0 && B <= 65535 && S > 0 && S % 4 == 0 && S <= 1024 && n_slots > 0 && (const void*)out != pool,
              "hct_gather_flip_labels: bad arguments (S must be a multiple of 4, at most 1024; at most 65535 volumes; the pool needs a slot)");
  HCT_REQUIRE(seg_aligned(pool, 4) && seg_aligned(out, 4), "hct_gather_flip_labels: pool and out must be 4-byte aligned");
  const int per_vol = S * S * (S / 4);
  const int want = (4096 + B - 1) / B;
  const dim3 grid((unsigned)std::max(1, std::min((per_vol + kSegThreads - 1) / kSegThreads, want)), (unsigned)B), block(kSegThreads);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gather_flip_labels_kernel, grid, block, 0, s, pool, slot, out, S, n_slots, flip, per_vol);
  HCT_CHECK_LAUNCH("hct_gather_flip_labels");
  return 0;
}

int hct_label_to_item(const float* ras, int d0, int d1, int d2, const int32_t* near, int m0, int m1, int m2, const int32_t* box, uint8_t* out,
                      int R0, int R1, int R2, int32_t* status, void* stream) {
  HCT_REQUIRE(ras && near && box && out && status, "hct_label_to_item: null argument");
  HCT_REQUIRE(d0 >= 1 && d1 >= 1 && d2 >= 1 && m0 >= 1 && m1 >= 1 && m2 >= 1 && R0 >= 1 && R1 >= 1 && R2 >= 1 && std::max({d0, d1, d2, m0, m1, m2, R0, R1, R2}) <= 1024,
              "hct_label_to_item: every axis must lie in [1, 1024]");
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_hip(hipMemsetAsync(status, 0, sizeof(int32_t), s), "hct_label_to_item (status)")) return rc;
  const int64_t total = (int64_t)R0 * R1 * R2;
  const int grid = (int)std::min<int64_t>(4096, (total + kSegThreads - 1) / kSegThreads);
  hipLaunchKernelGGL(label_to_item_kernel, dim3(grid), dim3(kSegThreads), 0, s, ras, d0, d1, d2, near, m0, m1, m2, box, out, R0, R1, R2, status);
  HCT_CHECK_LAUNCH("hct_label_to_item");
  return 0;
}

}  // extern "C"
