// Multi-label fine-tuning loss: sigmoid + binary cross-entropy over a [B, T] table of labels with gaps (hct_sigmoid_bce).
// An addition of this build: the reference trains one binary model per label and has no such loss.
//
// Three short launches on the caller's stream, all plain fp32 loads and stores, no atomics:
//   partial   grid (column blocks, row blocks): a block is ry x cx threads, cx = the power of two that covers T (at most 256),
//             ry = 256 / cx.  Thread (i, j) owns column j of its column block and the rows r0 + i, r0 + i + ry, ... of its row
//             block, sums their loss terms and counts the valid ones in that order; the ry sums of a column are folded by a
//             halving tree through LDS.  One (sum, count) per row block and column goes to the workspace.
//   finalize  one block: per column the row blocks in index order (double), label_loss, then the columns tid, tid + 256, ...
//             and a halving tree: the loss and the number n of valid entries (kept in the workspace for the gradient).
//   gradient  a grid-stride pass over the B * T elements, one element per thread and trip, scaled by 1 / max(n, 1) and by g.
// A fine-tuning batch is 64 x 14 elements: one partial block, the finalize block, four gradient blocks.
#include "common.h"
#include "prof.h"

#include <algorithm>

namespace hct {
namespace {

constexpr int kBceThreads = 256;
constexpr int kBceRowTrips = 4;       // rows a thread takes before its column is shared out over another row block
constexpr int kBceMaxRowBlocks = 64;  // partial (sum, count) pairs per column
constexpr int kBceGradBlocks = 256;   // gradient pass: blocks of one element per thread and trip (one per CU)
constexpr size_t kBceHead = 16;       // workspace head: the valid-entry count (int64), padded

struct BceShape {
  int cx, ry, col_blocks, chunk, row_blocks;
};

BceShape bce_shape(int B, int T) {
  BceShape s;
  s.cx = 1;
  while (s.cx < T && s.cx < kBceThreads) s.cx <<= 1;
  s.ry = kBceThreads / s.cx;
  s.col_blocks = (T + s.cx - 1) / s.cx;
  const int per_block = s.ry * kBceRowTrips;
  const int want = (int)std::min<int64_t>(kBceMaxRowBlocks, ((int64_t)B + per_block - 1) / per_block);
  s.chunk = (int)(((int64_t)B + want - 1) / want);
  s.row_blocks = (int)(((int64_t)B + s.chunk - 1) / s.chunk);
  return s;
}

// L = log1p(exp(-|x|)): softplus(x) = max(x, 0) + L, softplus(-x) = max(-x, 0) + L
__device__ __forceinline__ float bce_term(float x, float y, float w) {
  const float L = log1pf(expf(-fabsf(x)));
  // (1 - y) x + (1 + (w - 1) y) softplus(-x), written as (1 - y) softplus(x) + w y softplus(-x): the same value without the
  // cancellation of x against softplus(-x) at a negative logit
  return (1.0f - y) * (fmaxf(x, 0.0f) + L) + w * y * (fmaxf(-x, 0.0f) + L);
}

__global__ void __launch_bounds__(kBceThreads) bce_partial_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                                  const float* __restrict__ pos_weight, int B, int T, int cx, int chunk,
                                                                  int need_loss, float* __restrict__ psum, int* __restrict__ pcnt) {
  __shared__ float ssum[kBceThreads];
  __shared__ int scnt[kBceThreads];
  const int tid = threadIdx.x, ry = kBceThreads / cx;
  const int j = tid & (cx - 1), i = tid / cx;
  const int64_t t = (int64_t)blockIdx.x * cx + j;
  const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = r0 + chunk < (int64_t)B ? r0 + chunk : (int64_t)B;
  float acc = 0.0f;
  int cnt = 0;
  if (t < T) {
    const float w = pos_weight ? pos_weight[t] : 1.0f;
    for (int64_t r = r0 + i; r < r1; r += ry) {
      const size_t e = (size_t)r * T + t;
      const float y = target[e];
      if (y >= 0.0f) {
        ++cnt;
        if (need_loss) acc += bce_term(logits[e], y, w);
      }
    }
  }
  ssum[tid] = acc;
  scnt[tid] = cnt;
  __syncthreads();
  for (int o = ry >> 1; o > 0; o >>= 1) {
    if (i < o) {
      ssum[tid] += ssum[tid + o * cx];
      scnt[tid] += scnt[tid + o * cx];
    }
    __syncthreads();
  }
  if (i == 0 && t < T) {
    psum[(size_t)blockIdx.y * T + t] = ssum[tid];
    pcnt[(size_t)blockIdx.y * T + t] = scnt[tid];
  }
}

__global__ void __launch_bounds__(kBceThreads) bce_finalize_kernel(const float* __restrict__ psum, const int* __restrict__ pcnt,
                                                                   int row_blocks, int T, float* __restrict__ loss,
                                                                   float* __restrict__ label_loss, long long* __restrict__ count) {
  __shared__ double ssum[kBceThreads];
  __shared__ long long scnt[kBceThreads];
  const int tid = threadIdx.x;
  double acc = 0.0;
  long long cnt = 0;
  for (int t = tid; t < T; t += kBceThreads) {
    double s = 0.0;
    long long c = 0;
    for (int rb = 0; rb < row_blocks; ++rb) {
      s += (double)psum[(size_t)rb * T + t];
      c += pcnt[(size_t)rb * T + t];
    }
    if (label_loss) label_loss[t] = c ? (float)(s / (double)c) : 0.0f;
    acc += s;
    cnt += c;
  }
  ssum[tid] = acc;
  scnt[tid] = cnt;
  __syncthreads();
  for (int o = kBceThreads >> 1; o > 0; o >>= 1) {
    if (tid < o) {
      ssum[tid] += ssum[tid + o];
      scnt[tid] += scnt[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const long long n = scnt[0];
    if (loss) loss[0] = (float)(ssum[0] / (double)(n > 0 ? n : 1));
    count[0] = n;
  }
}

__global__ void __launch_bounds__(kBceThreads) bce_grad_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                               const float* __restrict__ pos_weight, int64_t total, int T,
                                                               const float* __restrict__ dloss, const long long* __restrict__ count,
                                                               float* __restrict__ dlogits) {
  const long long n = count[0];
  // 1 / max(n, 1) first, then g: a loss scaled by g gives exactly g times the unscaled gradient's fp32 value
  const float inv_n = 1.0f / (float)(n > 0 ? n : 1), g = dloss ? dloss[0] : 1.0f;
  for (int64_t e = (int64_t)blockIdx.x * kBceThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBceThreads) {
    const float y = target[e];
    float d = 0.0f;
    if (y >= 0.0f) {
      const float x = logits[e], w = pos_weight ? pos_weight[e % T] : 1.0f;
      // s(|x|) = 1 / (1 + q), s(-|x|) = q / (1 + q), q = exp(-|x|): neither is formed as one minus the other
      const float q = expf(-fabsf(x)), big = 1.0f / (1.0f + q), small = q / (1.0f + q);
      const float sx = x >= 0.0f ? big : small, snx = x >= 0.0f ? small : big;
      d = ((1.0f - y) * sx - w * y * snx) * inv_n * g;
    }
    dlogits[e] = d;
  }
}

}  // namespace
}  // namespace hct

using namespace hct;

extern "C" {

size_t hct_sigmoid_bce_workspace_bytes(int B, int T) {
  if (B < 1 || T < 1) return 0;
  const BceShape s = bce_shape(B, T);
  return kBceHead + (size_t)s.row_blocks * (size_t)T * (sizeof(float) + sizeof(int));
}

int hct_sigmoid_bce(const float* logits, const float* target, const float* pos_weight, int B, int T, const float* dloss, float* loss,
                    float* label_loss, float* dlogits, void* workspace, size_t workspace_bytes, void* stream) {
  HCT_REQUIRE(logits && target && B >= 1 && T >= 1 && (loss || label_loss || dlogits),
              "hct_sigmoid_bce: bad arguments (logits and target [B, T] with B, T >= 1, and at least one of loss, label_loss, dlogits)");
  const size_t need = hct_sigmoid_bce_workspace_bytes(B, T);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7u)) {
    set_error("hct_sigmoid_bce: workspace too small or not 8-byte aligned (%zu < %zu)", workspace_bytes, need);
    return HCT_E_WORKSPACE;
  }
  const BceShape sh = bce_shape(B, T);
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = (int64_t)B * T;
  long long* count = (long long*)workspace;
  float* psum = (float*)((char*)workspace + kBceHead);
  int* pcnt = (int*)(psum + (size_t)sh.row_blocks * T);
  const int need_loss = (loss || label_loss) ? 1 : 0;
  ProfScope ps(PROF_BCE, (double)total, s, (double)total * (need_loss ? 8.0 : 4.0) + (dlogits ? (double)total * 12.0 : 0.0));
  hipLaunchKernelGGL(bce_partial_kernel, dim3(sh.col_blocks, sh.row_blocks), dim3(kBceThreads), 0, s, logits, target, pos_weight, B, T, sh.cx,
                     sh.chunk, need_loss, psum, pcnt);
  hipLaunchKernelGGL(bce_finalize_kernel, dim3(1), dim3(kBceThreads), 0, s, psum, pcnt, sh.row_blocks, T, loss, label_loss, count);
  if (dlogits) {
    const int grid = (int)std::min<int64_t>(kBceGradBlocks, (total + kBceThreads - 1) / kBceThreads);
    hipLaunchKernelGGL(bce_grad_kernel, dim3(grid), dim3(kBceThreads), 0, s, logits, target, pos_weight, total, T, dloss, count, dlogits);
  }
  HCT_CHECK_LAUNCH("hct_sigmoid_bce");
  return 0;
}

}  // extern "C"
