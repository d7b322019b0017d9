// Segmentation on the scan's own grid (hct_seg_to_native): the decoder's logits, read in TOKEN layout as hct_seg_predict reads
// them, are carried back through the loading chain's geometry (file -> RAS -> 1 mm -> foreground box -> item) onto the voxels of
// the file, blended trilinearly in fp32 and arg-maxed there.  An addition of this build: the reference has no per-voxel task.
//
// Geometry.  Every step of the forward chain is a per-axis map, so the host (headct_foundation_amd/native.py, float64) folds the
// whole of it into four tables per FILE axis a (length n_a): file index f reads item indices i0[f], i1[f] of ITEM axis o
// (perm[o] == a) with weight w[f] on i1, and inside[f] says whether f lies in the foreground box at all.  A voxel that is outside
// on any axis is background (class 0): nothing was predicted there.  The item is the cube [S, S, S], S = G * P, of the token
// layout (segmentation.hip): element (t0, t1, t2) of class c is column c * P^3 + v of row first + l, and both l and v are sums
// of one term per axis -- off(o, t) = (t / P) * tok[o] * ld + (t % P) * vox[o], tok = {G^2, G, 1}, vox = {P^2, P, 1} -- so a tap's
// address is a sum of three per-axis offsets.
//
// Work split.  A file row (fixed j, k; i contiguous) has constant taps and weights on the two other axes, and neighbouring rows
// j, j + 1 of one slice k mostly read the SAME two item rows (a 0.45 mm file axis crosses an item voxel in four steps).  One wave
// (a workgroup of 64 threads) takes a slice k and kNatRows consecutive rows j.  It keeps two item rows in LDS, each K * S floats
// ([c][t], so that neighbouring lanes, whose i0 differ by 0 or 1, read neighbouring words or the same one) and each already
// blended along k: slot A for the row at j0, slot B for the row at j1.  Stepping to the next j refills a slot only when its
// item row changes, and a row that moves from j1 to j0 changes slots without a load.  These gathers are the only global reads of
// logits (2 * K * S two-tap loads per refilled pair), scattered 2- or 4-byte loads out of the cache-resident logits; everything
// after them runs out of LDS.  Every lane then blends along j and i per class (4 LDS reads, 3 lerps), takes the arg-max (strictly
// greater: the lowest class wins a tie, hct_seg_predict's rule) and stores int16, lane by lane contiguous.  A lerp is
// a + w * (b - a), compiled without contraction: w = 0 gives a exactly.  Rows that are outside on j or k are written as zeros
// without touching the logits.
//
// Reductions.  Per thread and class: voxels, TP, FP, FN (labels uint8 in file order, 255 and anything >= K = ignore), summed over
// the lanes by the xor butterfly into one partial per workgroup; native_fold_kernel adds the partials in a fixed order into int64.
// Integer sums: the result does not depend on launch order, a repeated call is bit-equal.
#include "common.h"
#include "prof.h"

#include <algorithm>

namespace hct {
namespace {

constexpr int kNatThreads = kWave;   // one wave per workgroup: its barrier costs nothing, and 20 of them fit a CU at K = 6
constexpr int kNatRows = 16;         // consecutive rows j of one slice per work item
constexpr int kNatMaxK = 16;
constexpr int kNatMaxBlocks = 8192;  // workgroups (= partials) per call: 8 waves on each SIMD of 256 CUs
constexpr int kNatMaxAxis = 1024;
constexpr int kNatMaxRow = 8192;     // K * S: two rows of that many floats are the 64 KiB of LDS a workgroup may ask for
constexpr int kFoldThreads = 256;

struct NatGeom {
  int first, G, P, S, P3;
  int oi, oj, ok;  // the item axis that file axis i / j / k feeds
  int ni, nj, nk;
  // element offset of index t on item axis o, without the class and the leading rows
  __device__ __forceinline__ int64_t off(int o, int t, int64_t ld) const {
    const int q = t / P, r = t - q * P;
    const int tok = o == 0 ? G * G : o == 1 ? G : 1, vox = o == 0 ? P * P : o == 1 ? P : 1;
    return (int64_t)q * tok * ld + (int64_t)r * vox;
  }
};

__device__ __forceinline__ float nat_lerp(float a, float b, float w) { return a + w * (b - a); }
__device__ __forceinline__ int nat_clamp(int v, int hi) { return min(max(v, 0), hi); }

// slot[c][t] = the logits of item row (tj on axis oj) blended along k, for every class c and every t on axis oi
template <typename T>
__device__ __forceinline__ void nat_fill(float* __restrict__ slot, const T* __restrict__ base, int64_t ld, const NatGeom& g, int K, int tj,
                                         int64_t ok0, int64_t ok1, float wk) {
  const int64_t oj = g.off(g.oj, tj, ld);
  for (int e = threadIdx.x; e < K * g.S; e += kNatThreads) {
    const int c = e / g.S, t = e - c * g.S;
    const T* p = base + (int64_t)c * g.P3 + g.off(g.oi, t, ld) + oj;
    slot[e] = nat_lerp(to_f32(p[ok0]), to_f32(p[ok1]), wk);
  }
}

template <typename T, int KT>
__global__ void __launch_bounds__(kNatThreads) native_kernel(const T* __restrict__ logits, int64_t ld, NatGeom g, int K,
                                                             const int32_t* __restrict__ i0, const int32_t* __restrict__ i1,
                                                             const float* __restrict__ w, const uint8_t* __restrict__ inside,
                                                             const uint8_t* __restrict__ labels, int16_t* __restrict__ pred,
                                                             int* __restrict__ partial) {
  extern __shared__ float lds[];  // two slots of K * S floats
  int cnt[4 * KT];  // [4 k + 0 / 1 / 2 / 3] = voxels / TP / FP / FN of class k
#pragma unroll
  for (int q = 0; q < 4 * KT; ++q) cnt[q] = 0;
  const int tid = threadIdx.x, S = g.S, hi = S - 1;
  // the tables of the three file axes lie one after the other: i, then j, then k
  const int bj = g.ni, bk = g.ni + g.nj;
  const int chunks = (g.nj + kNatRows - 1) / kNatRows, items = chunks * g.nk;
  const T* base = logits + (int64_t)g.first * ld;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {  // everything in this loop but the voxel loop is uniform over the wave
    const int k = item / chunks, jbeg = (item - k * chunks) * kNatRows, jend = min(g.nj, jbeg + kNatRows);
    const bool in_k = inside[bk + k] != 0;
    const int k0 = nat_clamp(i0[bk + k], hi), k1 = nat_clamp(i1[bk + k], hi);
    const float wk = w[bk + k];
    const int64_t ok0 = g.off(g.ok, k0, ld), ok1 = g.off(g.ok, k1, ld);
    float *A = lds, *B = lds + K * S;
    int curA = -1, curB = -1;  // the item rows the slots hold (of this slice)
    for (int j = jbeg; j < jend; ++j) {
      const bool in_row = in_k && inside[bj + j] != 0;
      float wj = 0.0f;
      if (in_row) {
        const int j0 = nat_clamp(i0[bj + j], hi), j1 = nat_clamp(i1[bj + j], hi);
        wj = w[bj + j];
        bool needA = curA != j0, needB = curB != j1;
        if (needA || needB) {
          __syncthreads();  // the lanes have read the slots for the row before
          if ((needA && curB == j0) || (needB && curA == j1)) {  // a row moves from j1 to j0 (or back, under a flip): the slots change roles
            float* s = A;
            A = B;
            B = s;
            const int c = curA;
            curA = curB;
            curB = c;
          }
          if (curA != j0) nat_fill<T>(A, base, ld, g, K, j0, ok0, ok1, wk);
          if (curB != j1) nat_fill<T>(B, base, ld, g, K, j1, ok0, ok1, wk);
          curA = j0;
          curB = j1;
          __syncthreads();
        }
      }
      const int64_t out = ((int64_t)k * g.nj + j) * g.ni;
      for (int i = tid; i < g.ni; i += kNatThreads) {
        int a = 0;
        if (in_row && inside[i] != 0) {
          const int t0 = nat_clamp(i0[i], hi), t1 = nat_clamp(i1[i], hi);
          const float wi = w[i];
          float m = nat_lerp(nat_lerp(A[t0], B[t0], wj), nat_lerp(A[t1], B[t1], wj), wi);
#pragma unroll
          for (int c = 1; c < KT; ++c)
            if (c < K) {
              const float* a_ = A + c * S;
              const float* b_ = B + c * S;
              const float v = nat_lerp(nat_lerp(a_[t0], b_[t0], wj), nat_lerp(a_[t1], b_[t1], wj), wi);
              if (v > m) {  // strictly greater: ties stay with the lowest class
                m = v;
                a = c;
              }
            }
        }
        pred[out + i] = (int16_t)a;
        const int y = labels ? (int)labels[out + i] : 255;
#pragma unroll
        for (int c = 0; c < KT; ++c)
          if (c < K) {
            const bool isa = a == c, isy = y == c;
            cnt[4 * c] += isa ? 1 : 0;
            if (y < K) {
              cnt[4 * c + 1] += (isa && isy) ? 1 : 0;
              cnt[4 * c + 2] += (isa && !isy) ? 1 : 0;
              cnt[4 * c + 3] += (!isa && isy) ? 1 : 0;
            }
          }
      }
    }
    __syncthreads();  // the next item starts with empty slots
  }
#pragma unroll
  for (int q = 0; q < 4 * KT; ++q)
    if (q < 4 * K) {
      int v = cnt[q];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (tid == 0) partial[(size_t)blockIdx.x * 4 * K + q] = v;
    }
}

// class_voxels[c] and counts[c][0 .. 2] out of the workgroups' partials: block q sums quantity q, thread t the partials t, t + 256,
// ..., then a halving tree over the threads
__global__ void __launch_bounds__(kFoldThreads) native_fold_kernel(const int* __restrict__ partial, int K, int nb, long long* __restrict__ class_voxels,
                                                                   long long* __restrict__ counts) {
  __shared__ long long sum[kFoldThreads];
  const int q = blockIdx.x, tid = threadIdx.x;
  long long v = 0;
  for (int b = tid; b < nb; b += kFoldThreads) v += partial[(size_t)b * 4 * K + q];
  sum[tid] = v;
  __syncthreads();
  for (int o = kFoldThreads >> 1; o > 0; o >>= 1) {
    if (tid < o) sum[tid] += sum[tid + o];
    __syncthreads();
  }
  if (tid != 0) return;
  const int c = q / 4, s = q - 4 * c;
  if (s == 0)
    class_voxels[c] = sum[0];
  else if (counts)
    counts[3 * c + s - 1] = sum[0];
}

int native_blocks(int nj, int nk) { return (int)std::min<int64_t>(kNatMaxBlocks, (int64_t)((nj + kNatRows - 1) / kNatRows) * nk); }

int native_check_shape(const char* what, int T, int first, int G, int P, int K, int64_t ld, int ni, int nj, int nk) {
  HCT_REQUIRE(G >= 1 && P >= 1 && K >= 2 && K <= kNatMaxK && first >= 0, "%s: bad shape (G %d, P %d, K %d in [2, %d], first %d)", what, G, P, K,
              kNatMaxK, first);
  HCT_REQUIRE((int64_t)G * P <= 1024, "%s: volume side G * P = %lld above 1024", what, (long long)G * P);
  HCT_REQUIRE((int64_t)K * G * P <= kNatMaxRow, "%s: K * G * P = %lld above %d (two rows of K * G * P floats are kept in LDS)", what,
              (long long)K * G * P, kNatMaxRow);
  HCT_REQUIRE((int64_t)T >= (int64_t)first + (int64_t)G * G * G, "%s: T %d < first %d + G^3 %lld", what, T, first, (long long)G * G * G);
  HCT_REQUIRE(ld >= (int64_t)K * P * P * P, "%s: row stride %lld < K * P^3 = %lld", what, (long long)ld, (long long)K * P * P * P);
  HCT_REQUIRE(ni >= 1 && nj >= 1 && nk >= 1 && std::max({ni, nj, nk}) <= kNatMaxAxis, "%s: file shape (%d, %d, %d): every axis must lie in [1, %d]", what,
              ni, nj, nk, kNatMaxAxis);
  return 0;
}

}  // namespace
}  // namespace hct

using namespace hct;

#define HCT_NAT_DISPATCH_K(K, ...)          \
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
      constexpr int KT = kNatMaxK;          \
      __VA_ARGS__;                          \
    }                                       \
  } while (0)

extern "C" {

size_t hct_seg_to_native_workspace_bytes(int ni, int nj, int nk, int K) {
  if (ni < 1 || nj < 1 || nk < 1 || std::max({ni, nj, nk}) > kNatMaxAxis || K < 2 || K > kNatMaxK) return 0;
  return (size_t)native_blocks(nj, nk) * 4 * K * sizeof(int);
}

int hct_seg_to_native(const void* logits, int dtype, int64_t ld, int T, int first, int G, int P, int K, const int32_t* i0, const int32_t* i1,
                      const float* w, const uint8_t* inside, int perm0, int perm1, int perm2, int ni, int nj, int nk, const uint8_t* labels,
                      int16_t* pred, int64_t* class_voxels, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  HCT_REQUIRE(logits && (dtype == HCT_F32 || dtype == HCT_BF16), "hct_seg_to_native: null logits or a dtype that is neither fp32 nor bf16");
  if (int rc = native_check_shape("hct_seg_to_native", T, first, G, P, K, ld, ni, nj, nk)) return rc;
  HCT_REQUIRE(i0 && i1 && w && inside, "hct_seg_to_native: null table (i0, i1, w and inside are all needed)");
  HCT_REQUIRE(pred && class_voxels, "hct_seg_to_native: null pred or class_voxels");
  HCT_REQUIRE(!counts || labels, "hct_seg_to_native: counts need labels");
  const int perm[3] = {perm0, perm1, perm2};
  int inv[3] = {-1, -1, -1};
  for (int o = 0; o < 3; ++o)
    if (perm[o] >= 0 && perm[o] < 3) inv[perm[o]] = o;
  HCT_REQUIRE(inv[0] >= 0 && inv[1] >= 0 && inv[2] >= 0, "hct_seg_to_native: perm (%d, %d, %d) is no permutation of 0, 1, 2", perm0, perm1, perm2);
  const size_t need = hct_seg_to_native_workspace_bytes(ni, nj, nk, K);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace % 4) != 0) {
    set_error("hct_seg_to_native: workspace too small or not 4-byte aligned (%zu < %zu)", workspace_bytes, need);
    return HCT_E_WORKSPACE;
  }
  const int S = G * P;
  const NatGeom g = {first, G, P, S, P * P * P, inv[0], inv[1], inv[2], ni, nj, nk};
  const int nb = native_blocks(nj, nk);
  const size_t lds = 2 * (size_t)K * S * sizeof(float);  // at most 64 KiB (native_check_shape)
  hipStream_t s = (hipStream_t)stream;
  const double voxels = (double)ni * nj * nk;
  ProfScope ps(PROF_SEG, voxels, s, (double)S * S * S * K * (double)dtype_size(dtype) + voxels * (2.0 + (labels ? 1.0 : 0.0)));
  HCT_DISPATCH_DTYPE(dtype, Tt, HCT_NAT_DISPATCH_K(K,
      hipLaunchKernelGGL((native_kernel<Tt, KT>), dim3(nb), dim3(kNatThreads), lds, s, (const Tt*)logits, ld, g, K, i0, i1, w, inside, labels, pred,
                         (int*)workspace)));
  hipLaunchKernelGGL(native_fold_kernel, dim3(4 * K), dim3(kFoldThreads), 0, s, (const int*)workspace, K, nb, (long long*)class_voxels,
                     (long long*)counts);
  HCT_CHECK_LAUNCH("hct_seg_to_native");
  return 0;
}

}  // extern "C"
