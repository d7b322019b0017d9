// Inference-side kernels of a trained encoder: volume-to-volume retrieval and attention maps.
//
// hct_topk_dot: for every query row the k largest dot products with the rows of a gallery, without ever forming the [Q, G] score
// matrix.  q and g hold unit vectors (hct_l2norm_rows_fwd), so a dot product is a cosine.
//
//   Geometry.  A workgroup of four waves owns 64 queries (16 per wave) and one CHUNK of gallery rows; the grid is
//   (ceil(Q / 64), chunks).  chunks = min(ceil(G / kChunkRows), max(1, kMaxGroups / ceil(Q / 64))) depends on (Q, G) only.
//   Scores.  bf16 with D % 32 == 0 and 16-byte-aligned rows: mfma_f32_16x16x32_bf16 with the GALLERY as the "A" operand and the
//   queries as the "B" operand, fragments read straight from global memory (lane l reads 16 contiguous bytes of row l & 15 at
//   k = 8 (l >> 4), as lora.hip does).  Lane l then holds, for query l & 15, the scores of gallery rows 4 (l >> 4) + e, e < 4, of
//   each of the four 16-row subtiles of a 64-row tile: one query's 64 scores of a tile sit in 4 lanes x 16 registers.
//   Everything else (fp32, D % 4 == 0): the same thread-to-(query, row) map, every score a sequential fmaf chain over D.
//   Either way a score is summed over D in an order that does not depend on where the row sits in its tile or chunk (the MFMA
//   treats its 256 outputs alike, k-steps run in ascending order), so bitwise-equal gallery rows give bitwise-equal scores.
//   Selection.  A candidate is the 64-bit key (order-preserving image of the fp32 score) << 32 | ~row: a larger key is a
//   better match, equal scores order by ascending row, and keys of distinct rows are distinct.  Every THREAD keeps a sorted list
//   of its k best keys in LDS (slot-major, so a wave's accesses are conflict-free), and inserts a candidate only if it beats
//   the list's current minimum, which it holds in a register.  No thread touches another thread's list: no atomics, no
//   barriers in the scan, nothing depends on timing.  At the end of the chunk the four lists of a query are merged (one barrier, then
//   one lane per query walks the four sorted lists) into the workspace ([Q, chunks, k] keys), and topk_merge_kernel picks the k
//   largest of a query's chunks * k keys by repeated arg-max.  Keys are totally ordered and unique, so the
//   result is the same for any chunking and bit-identical from call to call.
//
// hct_attention_row_probs: probs[b, h, r, :] = softmax_j(q[b, h, rows[r]] . k[b, h, j] dh^-1/2) from the qkv buffer of
// hct_attention_fwd, for a handful of query rows (the class token's, for attention maps).  One workgroup per (group of up to
// 8 rows, head, volume): K is read once per row group, logits / maximum / sum are fp32, reductions run in a fixed order.
#include <math.h>

#include "common.h"

using namespace hct;

namespace {

constexpr int kChunkRows = 1024;  // smallest gallery chunk (a multiple of the 64-row tile)
constexpr int kMaxGroups = 2048;  // chunks stop multiplying once the grid has this many workgroups
constexpr int kMaxK = 64;

typedef unsigned long long u64;

int topk_chunks(int Q, int64_t G) {
  const int64_t qb = ((int64_t)Q + 63) / 64;
  const int64_t by_rows = (G + kChunkRows - 1) / kChunkRows;
  const int64_t by_grid = kMaxGroups / qb > 1 ? kMaxGroups / qb : 1;
  const int64_t c = by_rows < by_grid ? by_rows : by_grid;
  return (int)(c < 1 ? 1 : c);
}

// rows per chunk: a multiple of 64 that covers G in `chunks` pieces
int64_t topk_chunk_rows(int64_t G, int chunks) { return ((G + chunks - 1) / chunks + 63) / 64 * 64; }

// order-preserving map of fp32 onto uint32 (-inf < ... < -0 < +0 < ... < +inf)
__device__ __forceinline__ uint32_t f32_orderable(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float f32_from_orderable(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
__device__ __forceinline__ u64 make_key(float score, int row) { return ((u64)f32_orderable(score) << 32) | (uint32_t)~(uint32_t)row; }

// A thread's sorted list of its k best keys: slot s of thread t at lds[s * 256 + t].  key 0 = empty (below every real key).
struct TopList {
  u64* lds;
  int k;
  u64 thr;  // lds[k - 1]: the key a candidate has to beat
  __device__ __forceinline__ void init(u64* base, int k_) {
    lds = base + threadIdx.x;
    k = k_;
    for (int s = 0; s < k; ++s) lds[s * 256] = 0;
    thr = 0;
  }
  __device__ __forceinline__ void offer(float score, int row) {
    const u64 key = make_key(score, row);
    if (key <= thr) return;
    int p = k - 1;
    while (p > 0) {
      const u64 up = lds[(p - 1) * 256];
      if (up >= key) break;
      lds[p * 256] = up;
      --p;
    }
    lds[p * 256] = key;
    thr = lds[(k - 1) * 256];
  }
  // After a workgroup barrier, by the lane with lane >> 4 == 0: the four sorted lists of a query (this thread's and those of
  // threads + 16, + 32, + 48, the same wave) merged into part [Q, chunks, k], best first.
  __device__ __forceinline__ void write_merged(u64* part, int q, int chunk, int chunks) const {
    u64* dst = part + ((size_t)q * chunks + chunk) * k;
    int pos[4] = {0, 0, 0, 0};
    u64 head[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) head[j] = lds[16 * j];
    for (int s = 0; s < k; ++s) {
      u64 best = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) best = head[j] > best ? head[j] : best;
      dst[s] = best;
      if (best == 0) continue;  // (the lists ran out: the remaining slots are empty)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (head[j] == best) {  // keys are unique: exactly one list advances
          ++pos[j];
          head[j] = pos[j] < k ? lds[pos[j] * 256 + 16 * j] : 0;
        }
      }
    }
  }
};

struct TopkArgs {
  const void* q;
  const void* g;
  const int32_t* exclude;
  u64* part;
  int Q, D, k, chunks;
  int64_t G, chunk_rows;
};

// bf16, D % 32 == 0, rows 16-byte aligned
__global__ void __launch_bounds__(256) topk_dot_mfma_kernel(TopkArgs a) {
  extern __shared__ u64 lists[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int q = blockIdx.x * 64 + wave * 16 + l15;
  const int qc = q < a.Q ? q : a.Q - 1;  // (queries past Q: a valid row is read, nothing is written)
  const int chunk = blockIdx.y;
  const int64_t row_begin = (int64_t)chunk * a.chunk_rows;
  const int64_t row_end = row_begin + a.chunk_rows < a.G ? row_begin + a.chunk_rows : a.G;
  const int excl = a.exclude ? a.exclude[qc] : -1;
  TopList list;
  list.init(lists, a.k);
  const bf16* qrow = (const bf16*)a.q + (size_t)qc * a.D + lq * 8;
  const bf16* gbase = (const bf16*)a.g + lq * 8;
  const int KS = a.D / 32;
  for (int64_t t0 = row_begin; t0 < row_end; t0 += 64) {
    const bf16* grow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int64_t r = t0 + 16 * j + l15;
      if (r >= a.G) r = a.G - 1;  // (rows past G: a valid row is read, its scores are never offered)
      grow[j] = gbase + (size_t)r * a.D;
    }
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 qf = *reinterpret_cast<const bf16x8*>(qrow + ks * 32);
      bf16x8 gf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) gf[j] = *reinterpret_cast<const bf16x8*>(grow[j] + ks * 32);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf[j], qf, acc[j], 0, 0, 0);
    }
    // acc[j][e] = score(query l15 of this wave, row t0 + 16 j + 4 lq + e): ascending rows in (j, e) order
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t r = t0 + 16 * j + 4 * lq + e;
        if (r < row_end && r != excl) list.offer(acc[j][e], (int)r);
      }
    }
  }
  __syncthreads();
  if (lq == 0 && q < a.Q) list.write_merged(a.part, q, chunk, a.chunks);
}

// fp32 or bf16 with D % 4 == 0: the same thread-to-(query, row) map, a sequential fmaf chain per score
template <typename T>
__global__ void __launch_bounds__(256) topk_dot_plain_kernel(TopkArgs a) {
  extern __shared__ u64 lists[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int q = blockIdx.x * 64 + wave * 16 + l15;
  const int qc = q < a.Q ? q : a.Q - 1;
  const int chunk = blockIdx.y;
  const int64_t row_begin = (int64_t)chunk * a.chunk_rows;
  const int64_t row_end = row_begin + a.chunk_rows < a.G ? row_begin + a.chunk_rows : a.G;
  const int excl = a.exclude ? a.exclude[qc] : -1;
  TopList list;
  list.init(lists, a.k);
  const T* qrow = (const T*)a.q + (size_t)qc * a.D;
  for (int64_t r = row_begin + lq; r < row_end; r += 4) {
    const T* grow = (const T*)a.g + (size_t)r * a.D;
    float acc = 0.f;
    for (int d = 0; d < a.D; d += 4) {
      const f32x4 x = Vec4<T>::load(qrow + d), y = Vec4<T>::load(grow + d);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(x[e], y[e], acc);
    }
    if (r != excl) list.offer(acc, (int)r);
  }
  __syncthreads();
  if (lq == 0 && q < a.Q) list.write_merged(a.part, q, chunk, a.chunks);
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), o, 64), lo = __shfl_xor((uint32_t)v, o, 64);
    const u64 other = ((u64)hi << 32) | lo;
    v = other > v ? other : v;
  }
  return v;
}

// one wave per query: slot s of the output is the largest key below the one of slot s - 1 (keys are unique; 0 = empty)
__global__ void __launch_bounds__(64) topk_merge_kernel(const u64* __restrict__ part, int n_per_query, int k, float* __restrict__ scores,
                                                        int32_t* __restrict__ idx) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const u64* src = part + (size_t)q * n_per_query;
  u64 last = ~0ull;
  for (int s = 0; s < k; ++s) {
    u64 best = 0;
    for (int i = lane; i < n_per_query; i += 64) {
      const u64 key = src[i];
      if (key < last && key > best) best = key;
    }
    best = wave_max_u64(best);
    if (lane == 0) {
      scores[(size_t)q * k + s] = best ? f32_from_orderable((uint32_t)(best >> 32)) : -INFINITY;
      idx[(size_t)q * k + s] = best ? (int32_t)~(uint32_t)best : -1;
    }
    last = best;  // (0 once the keys run out: every later slot is empty)
  }
}

// ---- attention probabilities of chosen query rows ----------------------------------------------------------------------------
constexpr int kRowGroup = 8;

template <typename T>
__device__ __forceinline__ void load8(const T* p, float* out);
template <>
__device__ __forceinline__ void load8<float>(const float* p, float* out) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    out[e] = a[e];
    out[4 + e] = b[e];
  }
}
template <>
__device__ __forceinline__ void load8<bf16>(const bf16* p, float* out) {
  const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = (float)a[e];
}

// fixed-order block reduction of up to kRowGroup values per thread (256 threads): wave reduce, then the four wave results in order
template <bool MAX>
__device__ __forceinline__ void block_reduce_rows(float* v, int nr, float* red /* [4][kRowGroup] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = 0; r < nr; ++r) {
    const float w = MAX ? wave_max(v[r]) : wave_sum(v[r]);
    if (lane == 0) red[wave * kRowGroup + r] = w;
  }
  __syncthreads();
  for (int r = 0; r < nr; ++r) {
    float x = red[r];
    for (int w = 1; w < 4; ++w) x = MAX ? fmaxf(x, red[w * kRowGroup + r]) : x + red[w * kRowGroup + r];
    v[r] = x;
  }
  __syncthreads();
}

template <typename T>
__global__ void __launch_bounds__(256) attention_row_probs_kernel(const T* __restrict__ qkv, int N, int H, int dh, const int32_t* __restrict__ rows,
                                                                  int n_rows, float scale, float* __restrict__ probs) {
  __shared__ float qs[kRowGroup * 128];
  __shared__ float red[4 * kRowGroup];
  const int r0 = blockIdx.x * kRowGroup, h = blockIdx.y, b = blockIdx.z;
  const int nr = n_rows - r0 < kRowGroup ? n_rows - r0 : kRowGroup;
  const size_t tok_stride = (size_t)3 * H * dh;
  const T* base = qkv + (size_t)b * N * tok_stride + (size_t)h * dh;
  for (int i = threadIdx.x; i < nr * dh; i += 256) {
    const int r = i / dh, d = i - r * dh;
    int row = rows[r0 + r];
    row = row < 0 ? 0 : row >= N ? N - 1 : row;  // memory safety only: the caller validates the rows
    qs[r * 128 + d] = to_f32(base[(size_t)row * tok_stride + d]);
  }
  __syncthreads();
  float* out = probs + (((size_t)b * H + h) * n_rows + r0) * N;
  float m[kRowGroup];
#pragma unroll
  for (int r = 0; r < kRowGroup; ++r) m[r] = -INFINITY;
  for (int j = threadIdx.x; j < N; j += 256) {
    const T* kp = base + (size_t)j * tok_stride + (size_t)H * dh;
    float acc[kRowGroup];
#pragma unroll
    for (int r = 0; r < kRowGroup; ++r) acc[r] = 0.f;
    for (int d = 0; d < dh; d += 8) {
      float kv[8];
      load8<T>(kp + d, kv);
#pragma unroll
      for (int r = 0; r < kRowGroup; ++r) {
        if (r < nr) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[r] = fmaf(qs[r * 128 + d + e], kv[e], acc[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kRowGroup; ++r) {
      if (r < nr) {
        const float l = acc[r] * scale;
        out[(size_t)r * N + j] = l;  // read back by this same thread below
        m[r] = fmaxf(m[r], l);
      }
    }
  }
  block_reduce_rows<true>(m, nr, red);
  float sum[kRowGroup];
#pragma unroll
  for (int r = 0; r < kRowGroup; ++r) sum[r] = 0.f;
  for (int j = threadIdx.x; j < N; j += 256) {
#pragma unroll
    for (int r = 0; r < kRowGroup; ++r) {
      if (r < nr) {
        const float e = expf(out[(size_t)r * N + j] - m[r]);
        out[(size_t)r * N + j] = e;
        sum[r] += e;
      }
    }
  }
  block_reduce_rows<false>(sum, nr, red);
  for (int j = threadIdx.x; j < N; j += 256) {
#pragma unroll
    for (int r = 0; r < kRowGroup; ++r) {
      if (r < nr) out[(size_t)r * N + j] = out[(size_t)r * N + j] / sum[r];
    }
  }
}

}  // namespace

extern "C" {

int hct_topk_dot_chunks(int Q, int64_t G) {
  if (Q <= 0 || G <= 0) return 0;
  return topk_chunks(Q, G);
}

size_t hct_topk_dot_workspace(int Q, int64_t G, int k) {
  if (Q <= 0 || G <= 0 || k < 1 || k > kMaxK) return 0;
  return (size_t)Q * topk_chunks(Q, G) * k * sizeof(u64);
}

int hct_topk_dot(const void* q, int Q, const void* g, int64_t G, int D, int dtype, const int32_t* exclude, int k, float* scores, int32_t* idx,
                 void* workspace, size_t workspace_bytes, void* stream) {
  HCT_REQUIRE(k >= 1 && k <= kMaxK, "hct_topk_dot: k must be in [1, %d] (%d)", kMaxK, k);
  HCT_REQUIRE(Q > 0 && G > 0 && G < (1ll << 31) && D > 0, "hct_topk_dot: bad shape (Q %d, G %lld, D %d)", Q, (long long)G, D);
  HCT_REQUIRE(dtype == HCT_F32 || dtype == HCT_BF16, "hct_topk_dot: dtype must be HCT_F32 or HCT_BF16");
  HCT_REQUIRE(D % 4 == 0, "hct_topk_dot: D must be a multiple of 4 (%d)", D);
  HCT_REQUIRE(q && g && scores && idx && workspace, "hct_topk_dot: null argument");
  HCT_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)g & 15) == 0 && ((uintptr_t)workspace & 7) == 0, "hct_topk_dot: q and g must be 16-byte aligned");
  const size_t need = hct_topk_dot_workspace(Q, G, k);
  if (workspace_bytes < need) {
    set_error("hct_topk_dot: workspace too small (%zu < %zu)", workspace_bytes, need);
    return HCT_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  TopkArgs a;
  a.q = q; a.g = g; a.exclude = exclude; a.part = (u64*)workspace;
  a.Q = Q; a.D = D; a.k = k; a.G = G;
  a.chunks = topk_chunks(Q, G);
  a.chunk_rows = topk_chunk_rows(G, a.chunks);
  const dim3 grid((Q + 63) / 64, a.chunks);
  const size_t lds = (size_t)256 * k * sizeof(u64);
  const void* fn = dtype == HCT_BF16 ? (D % 32 == 0 ? (const void*)topk_dot_mfma_kernel : (const void*)topk_dot_plain_kernel<bf16>)
                                      : (const void*)topk_dot_plain_kernel<float>;
  if (lds > 48 * 1024)  // k > 24: the lists need more LDS than a launch gets without asking (128 KB of the CU's 160 at k = 64)
    if (int rc = check_hip(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute(LDS)")) return rc;
  if (dtype == HCT_BF16 && D % 32 == 0) hipLaunchKernelGGL(topk_dot_mfma_kernel, grid, dim3(256), lds, s, a);
  else HCT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(topk_dot_plain_kernel<T>, grid, dim3(256), lds, s, a));
  HCT_CHECK_LAUNCH("hct_topk_dot");
  hipLaunchKernelGGL(topk_merge_kernel, dim3(Q), dim3(64), 0, s, (const u64*)workspace, a.chunks * k, k, scores, idx);
  return check_hip(hipGetLastError(), "hct_topk_dot (merge)");
}

int hct_attention_row_probs(const void* qkv, int B, int N, int H, int dh, int dtype, const int32_t* rows, int n_rows, float* probs, void* stream) {
  HCT_REQUIRE(B > 0 && N > 0 && H > 0 && n_rows > 0, "hct_attention_row_probs: bad shape (B %d, N %d, H %d, n_rows %d)", B, N, H, n_rows);
  HCT_REQUIRE(dh >= 8 && dh <= 128 && dh % 8 == 0, "hct_attention_row_probs: dh must be a multiple of 8 up to 128 (%d)", dh);
  HCT_REQUIRE(dtype == HCT_F32 || dtype == HCT_BF16, "hct_attention_row_probs: dtype must be HCT_F32 or HCT_BF16");
  HCT_REQUIRE(qkv && rows && probs, "hct_attention_row_probs: null argument");
  HCT_REQUIRE(((uintptr_t)qkv & 15) == 0, "hct_attention_row_probs: qkv must be 16-byte aligned");
  HCT_REQUIRE(H <= 65535 && B <= 65535, "hct_attention_row_probs: H and B must fit a grid dimension");
  const dim3 grid((n_rows + kRowGroup - 1) / kRowGroup, H, B);
  const float scale = 1.0f / sqrtf((float)dh);
  HCT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(attention_row_probs_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)qkv, N, H, dh, rows,
                                                  n_rows, scale, probs));
  return check_hip(hipGetLastError(), "hct_attention_row_probs");
}

}  // extern "C"
