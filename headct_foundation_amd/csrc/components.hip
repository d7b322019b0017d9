// Connected components of a mask on the scan's own grid (headct_foundation_amd/components.py): flag bytes of a class, 3-D labelling at
// connectivity 6 / 18 / 26, scipy's numbering, voxels per component, overlap of a component with another mask, removal of the
// components below a size, and the recount of a filtered prediction.  An addition of this build: the reference has no per-voxel task.
//
// Labelling (hct_cc_label): union-find over the voxels of the whole volume, in the output array itself.  label[v] = 1 + parent(v)
// on the mask and 0 off it; v = (k * nj + j) * ni + i.  Four launches, ordered by the kernel boundary alone:
//   runs     one wave per row (k, j): every mask voxel points at the first voxel of its run of consecutive mask voxels along i
//            (a ballot and a count of leading zeros per 64 voxels, the run's start carried from one 64 to the next);
//   merge    every mask voxel unites itself with the mask voxels among its 3 / 9 / 13 neighbours that come before it in memory and
//            lie in another row; a pair whose left-hand neighbours (v - 1, n - 1) are both on the mask is skipped, because those
//            two unite the same two runs.  Neighbours are spatial: an index outside [0, n_a) on any axis is no neighbour, so the
//            end of a row never meets the start of the next;
//   flatten  every run start, then every voxel, writes 1 + find(v).
// There is no tile phase in LDS: hct_cc_tile_dims reports the axis limit on every axis.
//
// INVARIANT: parent(v) <= v at every instant, for every mask voxel v.  The runs kernel establishes it (a run's start is not
// after its voxels); afterwards a slot changes only through atomicMin (merge) or by a store of find(v) <= v into v's own slot
// (flatten).  So a find, which follows x <- parent(x) until parent(x) == x, strictly decreases x and terminates, whatever the
// other workgroups do meanwhile.  No thread waits for a value another workgroup will write: no spin, no flag, no ticket.
//
// Union (merge).  Repeat: a <- find(a), b <- find(b); equal: done; let a > b; old <- atomicMin(&parent[a], b); old == a: a was a
// root and now hangs below b, done; else a <- old and go round again.  In the other case parent[a] holds min(old, b): either the
// link a -> old stays and b still has to meet old's tree, or a -> b has replaced it and old's tree, cut off from a, has to meet b:
// both are "unite old with b", which is what the next round does.  a + b falls strictly every round, so the loop ends.  A root is
// only ever hung below a SMALLER index, hence the root of a finished tree is the smallest linear index of its component, which
// does not depend on the order of the merges: the output is bit-equal from call to call although the kernel races.
//
// Stale reads are harmless.  Workgroups on different XCDs update `parent` at the same time and each XCD has its own L2, so a
// load may return a value the slot held earlier.  The loads of the merge and flatten kernels are relaxed agent-scope atomics (no
// vector L1, no register caching), but the argument needs no freshness.  Every value a slot ever held is an index <= v in v's
// final set: the slots only fall, and a replaced link is re-united by the thread that replaced it (above).  So a find over stale
// values still ends, at an index r of the same set whose slot ONCE said "root".  Whether it still does is decided by the
// atomicMin on r's slot, which executes at the memory side: the value it returns is the truth the loop goes on from.  A stale
// "root" costs a round, never a wrong merge.  No path is compressed while merges run (a compressing store could drop a link that
// no thread would restore); the flatten kernels run after the last merge, when the sets are final, and store only find(v) into
// v's own slot, an ancestor whichever value a concurrent reader sees.
//
// Numbering (hct_cc_compact).  v is a root iff label[v] == v + 1.  Chunks of 4096 voxels count their roots (one workgroup each), a
// second level scans 1024 chunk counts per workgroup, a third scans the second level's totals in one workgroup and writes n:
// a fixed-order prefix sum, no atomic counter, so component m is the m-th root in raster order -- scipy.ndimage.label's
// numbering.  Roots then take -(number), and in a last launch every other mask voxel reads its root's slot and stores the
// absolute value while the roots flip their own sign: a reader sees -m or +m, never anything else.
//
// Sizes and overlap: a wave reads 64 consecutive labels, splits them into runs of equal labels by a ballot, and the first lane of a
// run adds the run's count with one integer atomic (integer sums do not depend on order).  One label per wave, the first it met
// and every 64 voxels' first once that one is absent, is counted in a register instead and added once when it is replaced: without
// it the voxels of a large component put every wave's adds on one address (1.7 ms for 7 M voxels of one label, 106 ms for 12 M
// scattered ones).  Recount: hct_seg_to_native's counts (voxels, TP, FP, FN per class; a label >= K is ignore) from per-thread
// counters, a butterfly per wave, one partial per workgroup, folded in a fixed order.
#include "common.h"

#include <algorithm>

namespace hct {
namespace {

constexpr int kCcThreads = 256;
constexpr int kCcWaves = kCcThreads / kWave;
constexpr int kCcMaxAxis = 32768;
constexpr int64_t kCcMaxVox = 2147483646ll;  // 2^31 - 2: 1 + index fits an int32
constexpr int kCcMaxBlocks = 8192;            // grid-stride kernels: 8 waves on each SIMD of 256 CUs
constexpr int kCcTallyBlocks = 2048;          // sizes and overlap: fewer, longer waves, so that a wave's register count replaces more atomics
constexpr int kCcChunk = 4096;                // voxels per workgroup of the numbering
constexpr int kCcScan = 1024;                 // chunk counts per workgroup of the second level
constexpr int kCcMaxK = 16;

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// label holds 1 + parent: follows the parents from x to the index whose slot says "root"
__device__ __forceinline__ int cc_find(const int* label, int x) {
  for (;;) {
    const int q = cc_load(label + x) - 1;
    if (q >= x) return x;  // q == x; ">" cannot happen (the invariant) and would end the walk all the same
    x = q;
  }
}

__device__ __forceinline__ void cc_union(int* label, int a, int b) {
  for (;;) {
    a = cc_find(label, a);
    b = cc_find(label, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(label + a, b + 1) - 1;
    if (old == a) return;
    a = old;
  }
}

__global__ void __launch_bounds__(kCcThreads) cc_masks_kernel(const int16_t* __restrict__ pred, const uint8_t* __restrict__ labels, int64_t nvox, int c,
                                                              uint8_t* __restrict__ flags) {
  for (int64_t v = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * kCcThreads) {
    unsigned f = pred[v] == c ? 1u : 0u;
    if (labels) {
      const int y = labels[v];
      if (y == 255) f = 0;
      f |= y == c ? 2u : 0u;
    }
    flags[v] = (uint8_t)f;
  }
}

// one wave per row: label = 1 + (first voxel of the run) on the mask, 0 off it
__global__ void __launch_bounds__(kCcThreads) cc_runs_kernel(const uint8_t* __restrict__ flags, int bit, int64_t rows, int ni, int* __restrict__ label) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int64_t row = (int64_t)blockIdx.x * kCcWaves + wave; row < rows; row += (int64_t)gridDim.x * kCcWaves) {
    const int64_t r0 = row * ni;
    int carry = 0;  // the start of the run a mask voxel at `base` belongs to
    for (int base = 0; base < ni; base += kWave) {
      const int i = base + lane;
      const bool m = i < ni && (flags[r0 + i] & bit) != 0;
      const unsigned long long on = __ballot(m);
      const unsigned long long off_below = ~on & ((1ull << lane) - 1ull);
      const int start = off_below ? base + 64 - __clzll((long long)off_below) : carry;
      if (i < ni) label[r0 + i] = m ? (int)(r0 + start) + 1 : 0;
      const int last = __shfl(start, kWave - 1, kWave);
      carry = (on >> (kWave - 1)) ? last : base + kWave;
    }
  }
}

// This kernel and cc_flatten_kernel give a row (k, j) to a workgroup and stride its threads over i, which spares a 64-bit division
// per voxel and keeps the accesses of a row contiguous at a scan's 512 voxels per row.  A volume much narrower than 256 along i
// (the (300, 1, 1) test case at the extreme) leaves most lanes idle: correct, and slow only where there is little to do.
__global__ void __launch_bounds__(kCcThreads) cc_merge_kernel(const uint8_t* __restrict__ flags, int bit, int nk, int nj, int ni, int reach,
                                                              int* __restrict__ label) {
  const int64_t rows = (int64_t)nk * nj;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int k = (int)(row / nj), j = (int)(row - (int64_t)k * nj);
    const int64_t r0 = row * ni;
    for (int i = threadIdx.x; i < ni; i += kCcThreads) {
      if (!(flags[r0 + i] & bit)) continue;
      const bool left = i > 0 && (flags[r0 + i - 1] & bit) != 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {  // the rows before this one: (k, j - 1), (k - 1, j - 1), (k - 1, j), (k - 1, j + 1)
        const int dk = q == 0 ? 0 : -1, dj = q == 0 ? -1 : q - 2;
        const int far = (dk != 0) + (dj != 0);
        if (far > reach || k + dk < 0 || j + dj < 0 || j + dj >= nj) continue;
        const int64_t n0 = (row + (int64_t)dk * nj + dj) * ni;
#pragma unroll
        for (int di = -1; di <= 1; ++di) {
          const int x = i + di;
          if (far + (di != 0) > reach || x < 0 || x >= ni) continue;
          if (!(flags[n0 + x] & bit)) continue;
          if (left && x > 0 && (flags[n0 + x - 1] & bit)) continue;  // (i - 1) and (x - 1) unite the same two runs
          cc_union(label, (int)(r0 + i), (int)(n0 + x));
        }
      }
    }
  }
}

// starts_only: the first voxel of every run; else every voxel (two hops after the run starts are flat)
__global__ void __launch_bounds__(kCcThreads) cc_flatten_kernel(const uint8_t* __restrict__ flags, int bit, int64_t rows, int ni, int starts_only,
                                                                int* __restrict__ label) {
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t r0 = row * ni;
    for (int i = threadIdx.x; i < ni; i += kCcThreads) {
      if (!(flags[r0 + i] & bit)) continue;
      if (starts_only && i > 0 && (flags[r0 + i - 1] & bit)) continue;
      const int v = (int)(r0 + i);
      cc_store(label + v, cc_find(label, v) + 1);
    }
  }
}

__device__ __forceinline__ bool cc_is_root(const int* label, int64_t v, int64_t nvox) { return v < nvox && label[v] == (int)v + 1; }

__global__ void __launch_bounds__(kCcThreads) cc_count_kernel(const int* __restrict__ label, int64_t nvox, int* __restrict__ part) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const int64_t c0 = (int64_t)blockIdx.x * kCcChunk;
  int n = 0;
  for (int e = threadIdx.x; e < kCcChunk; e += kCcThreads) n += cc_is_root(label, c0 + e, nvox) ? 1 : 0;
  if (n) atomicAdd(&cnt, n);  // an integer sum in LDS: its order does not matter
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = cnt;
}

// exclusive scan of up to kCcScan values per workgroup, in place, in a fixed order; the workgroup's total goes to tot[blockIdx.x]
// (n_out != null: the single workgroup of the last level, which also writes the grand total)
__global__ void __launch_bounds__(kCcThreads) cc_scan_kernel(int* __restrict__ val, int n, int* __restrict__ tot, long long* __restrict__ n_out) {
  __shared__ int s[kCcThreads];
  constexpr int per = kCcScan / kCcThreads;
  const int b0 = blockIdx.x * kCcScan + threadIdx.x * per;
  int x[per], sum = 0;
#pragma unroll
  for (int q = 0; q < per; ++q) {
    x[q] = b0 + q < n ? val[b0 + q] : 0;
    sum += x[q];
  }
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < kCcThreads; o <<= 1) {  // Hillis-Steele over the threads' sums
    const int t = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  int run = s[threadIdx.x] - sum;
#pragma unroll
  for (int q = 0; q < per; ++q) {
    if (b0 + q < n) val[b0 + q] = run;
    run += x[q];
  }
  if (threadIdx.x == kCcThreads - 1) {
    if (tot) tot[blockIdx.x] = s[threadIdx.x];
    if (n_out) *n_out = s[threadIdx.x];
  }
}

// roots take -(their number): the chunk's base, plus the roots before them in the chunk
__global__ void __launch_bounds__(kCcThreads) cc_number_kernel(int* __restrict__ label, int64_t nvox, const int* __restrict__ part, const int* __restrict__ part2) {
  __shared__ int wsum[kCcWaves];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t c0 = (int64_t)blockIdx.x * kCcChunk;
  int base = part[blockIdx.x] + part2[blockIdx.x / kCcScan];
  for (int e0 = 0; e0 < kCcChunk; e0 += kCcThreads) {
    const int64_t v = c0 + e0 + threadIdx.x;
    const bool root = cc_is_root(label, v, nvox);
    const unsigned long long b = __ballot(root);
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
    for (int w = 0; w < kCcWaves; ++w) {
      before += w < wave ? wsum[w] : 0;
      all += wsum[w];
    }
    if (root) label[v] = -(base + before + 1);
    base += all;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kCcThreads) cc_renumber_kernel(int* __restrict__ label, int64_t nvox) {
  for (int64_t v = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * kCcThreads) {
    const int x = label[v];  // only this thread writes the slot
    if (x < 0) {
      cc_store(label + v, -x);
    } else if (x > 0) {
      const int m = cc_load(label + x - 1);  // the root's slot: -number, or +number once the root has flipped it
      label[v] = m < 0 ? -m : m;
    }
  }
}

__global__ void __launch_bounds__(kCcThreads) cc_zero_kernel(long long* __restrict__ out, int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kCcThreads) out[e] = 0;
}

// out[label] += voxels of the label (flags == null) or those of them whose flag has `bit`; one atomic per run of equal labels in a wave
__global__ void __launch_bounds__(kCcThreads) cc_tally_kernel(const int* __restrict__ label, const uint8_t* __restrict__ flags, int bit, int64_t nvox,
                                                              long long n, unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t step = (int64_t)gridDim.x * kCcThreads;
  int hot = 0;                    // the label this wave counts in a register (uniform over the wave): a large component would
  unsigned long long hot_cnt = 0;  // otherwise put every wave's adds on one address
  for (int64_t v0 = (int64_t)blockIdx.x * kCcThreads; v0 < nvox; v0 += step) {  // uniform over the workgroup: every lane reaches the ballots
    const int64_t v = v0 + threadIdx.x;
    int lab = v < nvox ? label[v] : 0;
    if (lab > n) lab = 0;
    const bool hit = lab > 0 && (!flags || (flags[v] & bit) != 0);
    const unsigned long long hits = __ballot(hit), on = __ballot(lab > 0), hot_lanes = hot ? __ballot(lab == hot) : 0ull;
    hot_cnt += (unsigned long long)__popcll(hits & hot_lanes);
    const int prev = __shfl_up(lab, 1, kWave);
    const bool head = lane == 0 || lab != prev;
    const unsigned long long heads = __ballot(head);
    if (head && lab > 0 && lab != hot) {
      const unsigned long long above = lane == kWave - 1 ? 0ull : heads >> (lane + 1);
      const int len = above ? __ffsll((long long)above) : kWave - lane;  // lanes of this run
      const unsigned long long span = (len == kWave ? ~0ull : ((1ull << len) - 1ull)) << lane;
      const int cnt = __popcll(hits & span);
      if (cnt) atomicAdd(out + lab, (unsigned long long)cnt);
    }
    if (!hot_lanes && on) {  // the register's label did not occur: hand its count over and take the first label of these 64 voxels
      if (lane == 0 && hot_cnt) atomicAdd(out + hot, hot_cnt);
      hot_cnt = 0;
      hot = __shfl(lab, __ffsll((long long)on) - 1, kWave);  // counted by its run above this time, in the register from the next 64 on
    }
  }
  if (lane == 0 && hot_cnt) atomicAdd(out + hot, hot_cnt);
}

__global__ void __launch_bounds__(kCcThreads) cc_remove_kernel(int16_t* __restrict__ pred, const int* __restrict__ label, const long long* __restrict__ sizes,
                                                               long long min_voxels, int64_t nvox) {
  for (int64_t v = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * kCcThreads) {
    const int lab = label[v];
    if (lab > 0 && sizes[lab] < min_voxels) pred[v] = 0;
  }
}

// *out += the labels 1 .. n whose size lies below min_voxels (out zeroed by the launch before); an integer sum
__global__ void __launch_bounds__(kCcThreads) cc_count_small_kernel(const long long* __restrict__ sizes, long long n, long long min_voxels,
                                                                    unsigned long long* __restrict__ out) {
  __shared__ unsigned int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  unsigned int c = 0;
  for (int64_t m = 1 + (int64_t)blockIdx.x * kCcThreads + threadIdx.x; m <= n; m += (int64_t)gridDim.x * kCcThreads) c += sizes[m] < min_voxels ? 1u : 0u;
  if (c) atomicAdd(&cnt, c);
  __syncthreads();
  if (threadIdx.x == 0 && cnt) atomicAdd(out, (unsigned long long)cnt);
}

template <int KT>
__global__ void __launch_bounds__(kCcThreads) cc_recount_kernel(const int16_t* __restrict__ pred, const uint8_t* __restrict__ labels, int64_t nvox, int K,
                                                                int* __restrict__ partial) {
  __shared__ int sw[kCcWaves][4 * KT];
  int cnt[4 * KT];  // [4 c + 0 / 1 / 2 / 3] = voxels / TP / FP / FN of class c
#pragma unroll
  for (int q = 0; q < 4 * KT; ++q) cnt[q] = 0;
  // a thread sees at most 2^31 / (blocks * 256) + 1 voxels: the counters cannot overflow
  for (int64_t v = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * kCcThreads) {
    const int a = pred[v], y = labels ? (int)labels[v] : 255;
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
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int q = 0; q < 4 * KT; ++q) {
    int v = cnt[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    if (lane == 0) sw[wave][q] = v;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < 4 * K; q += kCcThreads) {
    int v = 0;
#pragma unroll
    for (int w = 0; w < kCcWaves; ++w) v += sw[w][q];
    partial[(size_t)blockIdx.x * 4 * K + q] = v;
  }
}

// hct_seg_to_native's fold: block q sums quantity q over the workgroups' partials, thread t the partials t, t + 256, ..., then a halving tree
__global__ void __launch_bounds__(kCcThreads) cc_recount_fold_kernel(const int* __restrict__ partial, int K, int nb, long long* __restrict__ class_voxels,
                                                                     long long* __restrict__ counts) {
  __shared__ long long sum[kCcThreads];
  const int q = blockIdx.x, tid = threadIdx.x;
  long long v = 0;
  for (int b = tid; b < nb; b += kCcThreads) v += partial[(size_t)b * 4 * K + q];
  sum[tid] = v;
  __syncthreads();
  for (int o = kCcThreads >> 1; o > 0; o >>= 1) {
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

bool cc_shape_ok(int nk, int nj, int ni) {
  return nk >= 1 && nj >= 1 && ni >= 1 && std::max({nk, nj, ni}) <= kCcMaxAxis && (int64_t)nk * nj * ni <= kCcMaxVox;
}

int cc_check_shape(const char* what, int nk, int nj, int ni) {
  HCT_REQUIRE(cc_shape_ok(nk, nj, ni), "%s: shape (%d, %d, %d): every axis must lie in [1, %d] and the volume hold at most 2^31 - 2 voxels", what, nk, nj, ni,
              kCcMaxAxis);
  return 0;
}

int cc_check_nvox(const char* what, int64_t nvox) {
  HCT_REQUIRE(nvox >= 1 && nvox <= kCcMaxVox, "%s: %lld voxels outside [1, 2^31 - 2]", what, (long long)nvox);
  return 0;
}

int cc_check_ws(const char* what, const void* ws, size_t have, size_t need) {
  if (need && (!ws || have < need || ((uintptr_t)ws % 8) != 0)) {
    set_error("%s: workspace too small or not 8-byte aligned (%zu < %zu)", what, have, need);
    return HCT_E_WORKSPACE;
  }
  return 0;
}

int flat_blocks(int64_t n) { return (int)std::min<int64_t>(kCcMaxBlocks, std::max<int64_t>((n + kCcThreads - 1) / kCcThreads, 1)); }
int tally_blocks(int64_t n) { return std::min(flat_blocks(n), kCcTallyBlocks); }
int row_blocks(int64_t rows) { return (int)std::min<int64_t>(kCcMaxBlocks, std::max<int64_t>(rows, 1)); }
int chunks_of(int64_t nvox) { return (int)((nvox + kCcChunk - 1) / kCcChunk); }

}  // namespace
}  // namespace hct

using namespace hct;

#define HCT_CC_DISPATCH_K(K, ...)  \
  do {                             \
    if ((K) <= 2) {                \
      constexpr int KT = 2;        \
      __VA_ARGS__;                 \
    } else if ((K) <= 4) {         \
      constexpr int KT = 4;        \
      __VA_ARGS__;                 \
    } else if ((K) <= 8) {         \
      constexpr int KT = 8;        \
      __VA_ARGS__;                 \
    } else {                       \
      constexpr int KT = kCcMaxK;  \
      __VA_ARGS__;                 \
    }                              \
  } while (0)

extern "C" {

void hct_cc_tile_dims(int* tk, int* tj, int* ti) {
  if (tk) *tk = kCcMaxAxis;  // no tile phase: the only seams are the volume's faces
  if (tj) *tj = kCcMaxAxis;
  if (ti) *ti = kCcMaxAxis;
}

int hct_cc_masks(const int16_t* pred, const uint8_t* labels, int nk, int nj, int ni, int cls, uint8_t* flags, void* stream) {
  if (int rc = cc_check_shape("hct_cc_masks", nk, nj, ni)) return rc;
  HCT_REQUIRE(pred && flags, "hct_cc_masks: null pred or flags");
  HCT_REQUIRE(cls >= 0 && cls <= 254, "hct_cc_masks: class %d outside [0, 254] (255 marks voxels that count nowhere)", cls);
  const int64_t nvox = (int64_t)nk * nj * ni;
  hipLaunchKernelGGL(cc_masks_kernel, dim3(flat_blocks(nvox)), dim3(kCcThreads), 0, (hipStream_t)stream, pred, labels, nvox, cls, flags);
  HCT_CHECK_LAUNCH("hct_cc_masks");
  return 0;
}

size_t hct_cc_label_workspace_bytes(int nk, int nj, int ni) {
  (void)nk, (void)nj, (void)ni;
  return 0;  // the union-find lives in the output array
}

int hct_cc_label(const uint8_t* flags, int bit, int nk, int nj, int ni, int connectivity, int32_t* label, void* workspace, size_t workspace_bytes,
                 void* stream) {
  if (int rc = cc_check_shape("hct_cc_label", nk, nj, ni)) return rc;
  HCT_REQUIRE(flags && label, "hct_cc_label: null flags or label");
  HCT_REQUIRE(bit >= 1 && bit <= 255, "hct_cc_label: bit mask %d outside [1, 255]", bit);
  HCT_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "hct_cc_label: connectivity %d is none of 6, 18, 26", connectivity);
  HCT_REQUIRE(((uintptr_t)label % 4) == 0, "hct_cc_label: label is not 4-byte aligned");
  if (int rc = cc_check_ws("hct_cc_label", workspace, workspace_bytes, hct_cc_label_workspace_bytes(nk, nj, ni))) return rc;
  const int reach = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;  // how many coordinates of a neighbour may differ
  const int64_t rows = (int64_t)nk * nj;
  const int nb = row_blocks(rows), nbw = row_blocks((rows + kCcWaves - 1) / kCcWaves);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_runs_kernel, dim3(nbw), dim3(kCcThreads), 0, s, flags, bit, rows, ni, (int*)label);
  hipLaunchKernelGGL(cc_merge_kernel, dim3(nb), dim3(kCcThreads), 0, s, flags, bit, nk, nj, ni, reach, (int*)label);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(nb), dim3(kCcThreads), 0, s, flags, bit, rows, ni, 1, (int*)label);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(nb), dim3(kCcThreads), 0, s, flags, bit, rows, ni, 0, (int*)label);
  HCT_CHECK_LAUNCH("hct_cc_label");
  return 0;
}

size_t hct_cc_compact_workspace_bytes(int nk, int nj, int ni) {
  if (!cc_shape_ok(nk, nj, ni)) return 0;
  const int nb = chunks_of((int64_t)nk * nj * ni), nb2 = (nb + kCcScan - 1) / kCcScan;
  return align_up((size_t)nb * sizeof(int), 8) + align_up((size_t)nb2 * sizeof(int), 8);
}

int hct_cc_compact(int32_t* label, int nk, int nj, int ni, int64_t* n_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = cc_check_shape("hct_cc_compact", nk, nj, ni)) return rc;
  HCT_REQUIRE(label && n_out, "hct_cc_compact: null label or n_out");
  if (int rc = cc_check_ws("hct_cc_compact", workspace, workspace_bytes, hct_cc_compact_workspace_bytes(nk, nj, ni))) return rc;
  const int64_t nvox = (int64_t)nk * nj * ni;
  const int nb = chunks_of(nvox), nb2 = (nb + kCcScan - 1) / kCcScan;  // nb2 <= 512 <= kCcScan: one workgroup scans the top level
  int* part = (int*)workspace;
  int* part2 = (int*)((char*)workspace + align_up((size_t)nb * sizeof(int), 8));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_count_kernel, dim3(nb), dim3(kCcThreads), 0, s, (const int*)label, nvox, part);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(nb2), dim3(kCcThreads), 0, s, part, nb, part2, (long long*)nullptr);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(kCcThreads), 0, s, part2, nb2, (int*)nullptr, (long long*)n_out);
  hipLaunchKernelGGL(cc_number_kernel, dim3(nb), dim3(kCcThreads), 0, s, (int*)label, nvox, (const int*)part, (const int*)part2);
  hipLaunchKernelGGL(cc_renumber_kernel, dim3(flat_blocks(nvox)), dim3(kCcThreads), 0, s, (int*)label, nvox);
  HCT_CHECK_LAUNCH("hct_cc_compact");
  return 0;
}

int hct_cc_sizes(const int32_t* label, int64_t nvox, int64_t n, int64_t* sizes, void* stream) {
  if (int rc = cc_check_nvox("hct_cc_sizes", nvox)) return rc;
  HCT_REQUIRE(label && sizes, "hct_cc_sizes: null label or sizes");
  HCT_REQUIRE(n >= 0 && n <= nvox, "hct_cc_sizes: %lld components of %lld voxels", (long long)n, (long long)nvox);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_zero_kernel, dim3(flat_blocks(n + 1)), dim3(kCcThreads), 0, s, (long long*)sizes, n + 1);
  hipLaunchKernelGGL(cc_tally_kernel, dim3(tally_blocks(nvox)), dim3(kCcThreads), 0, s, (const int*)label, (const uint8_t*)nullptr, 0, nvox, (long long)n,
                     (unsigned long long*)sizes);
  HCT_CHECK_LAUNCH("hct_cc_sizes");
  return 0;
}

int hct_cc_overlap(const int32_t* label_a, int64_t n_a, const uint8_t* flags, int bit_b, int64_t nvox, int64_t* overlap, void* stream) {
  if (int rc = cc_check_nvox("hct_cc_overlap", nvox)) return rc;
  HCT_REQUIRE(label_a && flags && overlap, "hct_cc_overlap: null label, flags or overlap");
  HCT_REQUIRE(bit_b >= 1 && bit_b <= 255, "hct_cc_overlap: bit mask %d outside [1, 255]", bit_b);
  HCT_REQUIRE(n_a >= 0 && n_a <= nvox, "hct_cc_overlap: %lld components of %lld voxels", (long long)n_a, (long long)nvox);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_zero_kernel, dim3(flat_blocks(n_a + 1)), dim3(kCcThreads), 0, s, (long long*)overlap, n_a + 1);
  hipLaunchKernelGGL(cc_tally_kernel, dim3(tally_blocks(nvox)), dim3(kCcThreads), 0, s, (const int*)label_a, flags, bit_b, nvox, (long long)n_a,
                     (unsigned long long*)overlap);
  HCT_CHECK_LAUNCH("hct_cc_overlap");
  return 0;
}

int hct_cc_remove_small(int16_t* pred, const int32_t* label, const int64_t* sizes, int64_t min_voxels, int64_t nvox, void* stream) {
  if (int rc = cc_check_nvox("hct_cc_remove_small", nvox)) return rc;
  HCT_REQUIRE(pred && label && sizes, "hct_cc_remove_small: null pred, label or sizes");
  hipLaunchKernelGGL(cc_remove_kernel, dim3(flat_blocks(nvox)), dim3(kCcThreads), 0, (hipStream_t)stream, pred, (const int*)label, (const long long*)sizes,
                     (long long)min_voxels, nvox);
  HCT_CHECK_LAUNCH("hct_cc_remove_small");
  return 0;
}

int hct_cc_count_small(const int64_t* sizes, int64_t n, int64_t min_voxels, int64_t* out, void* stream) {
  HCT_REQUIRE(sizes && out, "hct_cc_count_small: null sizes or out");
  HCT_REQUIRE(n >= 0 && n <= kCcMaxVox, "hct_cc_count_small: %lld components outside [0, 2^31 - 2]", (long long)n);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_zero_kernel, dim3(1), dim3(kCcThreads), 0, s, (long long*)out, (int64_t)1);
  hipLaunchKernelGGL(cc_count_small_kernel, dim3(tally_blocks(std::max<int64_t>(n, 1))), dim3(kCcThreads), 0, s, (const long long*)sizes, (long long)n,
                     (long long)min_voxels, (unsigned long long*)out);
  HCT_CHECK_LAUNCH("hct_cc_count_small");
  return 0;
}

size_t hct_seg_recount_workspace_bytes(int nk, int nj, int ni, int K) {
  if (!cc_shape_ok(nk, nj, ni) || K < 2 || K > kCcMaxK) return 0;
  return (size_t)flat_blocks((int64_t)nk * nj * ni) * 4 * K * sizeof(int);
}

int hct_seg_recount(const int16_t* pred, const uint8_t* labels, int nk, int nj, int ni, int K, int64_t* class_voxels, int64_t* counts, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (int rc = cc_check_shape("hct_seg_recount", nk, nj, ni)) return rc;
  HCT_REQUIRE(K >= 2 && K <= kCcMaxK, "hct_seg_recount: K %d outside [2, %d]", K, kCcMaxK);
  HCT_REQUIRE(pred && class_voxels, "hct_seg_recount: null pred or class_voxels");
  HCT_REQUIRE(!counts || labels, "hct_seg_recount: counts need labels");
  if (int rc = cc_check_ws("hct_seg_recount", workspace, workspace_bytes, hct_seg_recount_workspace_bytes(nk, nj, ni, K))) return rc;
  const int64_t nvox = (int64_t)nk * nj * ni;
  const int nb = flat_blocks(nvox);
  hipStream_t s = (hipStream_t)stream;
  HCT_CC_DISPATCH_K(K, hipLaunchKernelGGL((cc_recount_kernel<KT>), dim3(nb), dim3(kCcThreads), 0, s, pred, labels, nvox, K, (int*)workspace));
  hipLaunchKernelGGL(cc_recount_fold_kernel, dim3(4 * K), dim3(kCcThreads), 0, s, (const int*)workspace, K, nb, (long long*)class_voxels, (long long*)counts);
  HCT_CHECK_LAUNCH("hct_seg_recount");
  return 0;
}

}  // extern "C"
