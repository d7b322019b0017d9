// Surface-distance metrics on the scan's own grid (HD, HD95, ASSD, NSD in millimetres; headct_foundation_amd/surface.py): the
// surface voxels of a predicted and an annotated mask, the exact Euclidean distance transform of each surface, and the
// statistics of one surface's distances to the other.  An addition of this build: the reference has no per-voxel task.
//
// Edges (hct_surface_edges).  For class c, P = (pred == c and label != 255), G = (label == c).  A mask voxel is a surface voxel
// unless all six face neighbours are mask voxels; a neighbour outside the volume is background, so the volume's border is
// surface.  One flag byte per voxel (bit 0: surface of P, bit 1: surface of G), the two counts, and the bounding box of every
// flagged voxel.  Both queries and features of everything below lie inside that box, and the box is convex along every axis, so
// the transform confined to it is exact: the minimising feature and the two intermediate points of the separable passes are inside.
//
// Transform (hct_edt3d).  Squared distance to the nearest flagged voxel, float64, in three passes along k, then j, then i:
//   pass k: a[k, j, i] = min over k' with a feature at (k', j, i) of ((k - k') s_k)^2
//   pass j: b[k, j, i] = min over j' of a[k, j', i] + ((j - j') s_j)^2
//   pass i: d[k, j, i] = min over i' of b[k, j, i'] + ((i - i') s_i)^2
// so a value is ((dk s_k)^2 + (dj s_j)^2) + (di s_i)^2 with every product and sum rounded once (the file is compiled without
// contraction), the order in which the float64 oracle adds them.  The direct form: no lower envelope, no intersection
// arithmetic that could pick the wrong parabola under rounding; a minimum does not depend on the order it is taken in.  A
// workgroup takes a tile of W neighbouring lines of the pass's axis (neighbours along i for the passes k and j, so that a
// global access covers W contiguous values; neighbours along j for the pass i, whose lines are contiguous themselves), loads
// their L partial values into LDS (L * W float64, at most 64 KiB) and every thread then takes the minimum over a line's L
// candidates for the outputs it owns: one LDS read (a broadcast over the lanes that share the candidate), a multiply by the
// spacing, a square, an add and a minimum per candidate.  The passes j and i run in place: a tile reads all of its cells
// before it writes any, and tiles are disjoint.  Where no voxel of the box is a feature every value stays +inf.
//
// Statistics (hct_surface_stats, hct_surface_select).  Both directions in one scan of the box: a voxel with bit 0 reads the
// field of G's surface, one with bit 1 the field of P's.  Counts, count of distances <= tau, sum and maximum go through
// per-thread accumulators, a halving tree over the workgroup, and a second tree over the workgroups' partials: a fixed order, no
// float atomics, a repeated call is bit-equal.  The order statistics of the 95th percentile come from an exact radix select over
// the bit patterns of the squared distances (non-negative doubles order as their integer images, and the square root is
// monotone): eight passes of eight bits, most significant first.  A pass counts, for each of the four wanted ranks (two per
// direction), the next byte of every value whose leading bytes equal the rank's prefix, in LDS histograms merged by integer
// atomics; a one-workgroup kernel then walks the 256 bins to the one that holds the rank.  No sort, no compaction.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace hct {
namespace {

constexpr int kSurfThreads = 256;
constexpr int kSurfMaxBlocks = 2048;   // workgroups (= partials) of a scan: 8 per CU
constexpr int kSurfMaxAxis = 32768;
constexpr int kEdtThreads = 256;
constexpr int kEdtMaxLine = 2048;      // longest line of the box on any axis
constexpr int kEdtTile = 4096;         // float64 values of a tile's LDS image where the width is not at a bound
constexpr int kEdtMinWidth = 4;        // lines per tile: kEdtTile / L held to [4, 32]; 2048 * 4 float64 = 64 KiB
constexpr int kEdtMaxWidth = 32;
constexpr int kSelPasses = 8;          // radix select: 8 passes of 8 bits over the 64-bit patterns
constexpr int kSelBins = 256;
constexpr int kSelSlots = 4;           // ranks: lo, hi of d(p -> G), then lo, hi of d(g -> P)

struct SurfBox {
  int k0, j0, i0, k1, j1, i1;  // [lo, hi) per axis
};

__device__ __forceinline__ bool in_p(const int16_t* pred, const uint8_t* labels, int64_t v, int c) { return labels[v] != 255 && pred[v] == c; }

// flags, and per workgroup [n_p, n_g, min k, min j, min i, max k, max j, max i] of the flagged voxels
__global__ void __launch_bounds__(kSurfThreads) surface_edges_kernel(const int16_t* __restrict__ pred, const uint8_t* __restrict__ labels, int nk, int nj,
                                                                     int ni, int c, uint8_t* __restrict__ flags, long long* __restrict__ partial) {
  __shared__ unsigned long long cnt[2];
  __shared__ int lo[3], hi[3];
  const int tid = threadIdx.x;
  if (tid < 2) cnt[tid] = 0;
  if (tid < 3) {
    lo[tid] = INT_MAX;
    hi[tid] = -1;
  }
  __syncthreads();
  unsigned long long np = 0, ng = 0;
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {-1, -1, -1};
  const int64_t rows = (int64_t)nk * nj, sk = (int64_t)nj * ni;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int k = (int)(row / nj), j = (int)(row - (int64_t)k * nj);
    const bool row_inner = k > 0 && k < nk - 1 && j > 0 && j < nj - 1;
    for (int i = tid; i < ni; i += kSurfThreads) {
      const int64_t v = row * ni + i;
      const int y = labels[v];
      const bool p = y != 255 && pred[v] == c, g = y == c;
      unsigned f = 0;
      if (p || g) {
        const bool inner = row_inner && i > 0 && i < ni - 1;  // a neighbour outside the volume is background
        bool pin = p && inner, gin = g && inner;
        if (inner) {
          const int64_t nb[6] = {v - 1, v + 1, v - ni, v + ni, v - sk, v + sk};
#pragma unroll
          for (int q = 0; q < 6; ++q) {
            if (pin) pin = in_p(pred, labels, nb[q], c);
            if (gin) gin = labels[nb[q]] == c;
          }
        }
        f = (p && !pin ? 1u : 0u) | (g && !gin ? 2u : 0u);
      }
      flags[v] = (uint8_t)f;
      if (f) {
        np += f & 1u;
        ng += f >> 1;
        mn[0] = min(mn[0], k), mn[1] = min(mn[1], j), mn[2] = min(mn[2], i);
        mx[0] = max(mx[0], k), mx[1] = max(mx[1], j), mx[2] = max(mx[2], i);
      }
    }
  }
  if (np) atomicAdd(&cnt[0], np);  // integer atomics in LDS: the result does not depend on their order
  if (ng) atomicAdd(&cnt[1], ng);
  if (mx[0] >= 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&lo[a], mn[a]);
      atomicMax(&hi[a], mx[a]);
    }
  }
  __syncthreads();
  if (tid < 2) partial[(size_t)blockIdx.x * 8 + tid] = (long long)cnt[tid];
  if (tid < 3) {
    partial[(size_t)blockIdx.x * 8 + 2 + tid] = lo[tid];
    partial[(size_t)blockIdx.x * 8 + 5 + tid] = hi[tid];
  }
}

// out[0 .. 7] = n_p, n_g, k0, j0, i0, k1, j1, i1 ([lo, hi); all zero where nothing is flagged)
__global__ void __launch_bounds__(kSurfThreads) surface_edges_fold_kernel(const long long* __restrict__ partial, int nb, long long* __restrict__ out) {
  __shared__ unsigned long long cnt[2];
  __shared__ int lo[3], hi[3];
  const int tid = threadIdx.x;
  if (tid < 2) cnt[tid] = 0;
  if (tid < 3) {
    lo[tid] = INT_MAX;
    hi[tid] = -1;
  }
  __syncthreads();
  for (int b = tid; b < nb; b += kSurfThreads) {
    const long long* p = partial + (size_t)b * 8;
    if (p[0]) atomicAdd(&cnt[0], (unsigned long long)p[0]);
    if (p[1]) atomicAdd(&cnt[1], (unsigned long long)p[1]);
    if (p[5] >= 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicMin(&lo[a], (int)p[2 + a]);
        atomicMax(&hi[a], (int)p[5 + a]);
      }
    }
  }
  __syncthreads();
  if (tid < 2) out[tid] = (long long)cnt[tid];
  if (tid < 3) {
    const bool any = hi[0] >= 0;
    out[2 + tid] = any ? lo[tid] : 0;
    out[5 + tid] = any ? hi[tid] + 1 : 0;
  }
}

// One pass of the transform over one tile: wc <= W neighbouring lines of L values.  Element e of the tile's LDS image is value l
// of line w with e = l * wc + w (fast_w: the lines are neighbours in memory) or e = w * L + l (the line itself is contiguous);
// its address is origin + l * ls + w * ws.  flags != null: the first pass, whose input is 0 at a feature and +inf elsewhere.
__global__ void __launch_bounds__(kEdtThreads) edt_pass_kernel(const uint8_t* __restrict__ flags, int bit, double* __restrict__ out, int64_t base, int L,
                                                               int64_t ls, int W, int64_t ws, int nw, int tiles_w, int64_t os, int fast_w, double s) {
  extern __shared__ double edt_lds[];
  const int outer = blockIdx.x / tiles_w, w0 = (blockIdx.x - outer * tiles_w) * W;
  const int wc = min(W, nw - w0), n = L * wc;
  const int64_t origin = base + (int64_t)outer * os + (int64_t)w0 * ws;
  const double inf = __builtin_huge_val();
  for (int e = threadIdx.x; e < n; e += kEdtThreads) {
    const int l = fast_w ? e / wc : e % L, w = fast_w ? e - l * wc : e / L;
    const int64_t a = origin + l * ls + w * ws;
    edt_lds[e] = flags ? ((flags[a] & bit) ? 0.0 : inf) : out[a];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += kEdtThreads) {
    const int l = fast_w ? e / wc : e % L, w = fast_w ? e - l * wc : e / L;
    const double* g = edt_lds + (fast_w ? w : w * L);
    const int cs = fast_w ? wc : 1;
    double m = inf, dl = (double)l;  // dl = l - l', exact
    for (int lp = 0; lp < L; ++lp) {
      const double t = dl * s;
      m = fmin(m, g[(size_t)lp * cs] + t * t);
      dl -= 1.0;
    }
    out[origin + l * ls + w * ws] = m;
  }
}

int edt_width(int L) { return std::min(kEdtMaxWidth, std::max(kEdtMinWidth, kEdtTile / std::max(L, 1))); }

// halving tree over the workgroup (fixed order): afterwards v[0] holds the result
template <typename T, typename Op>
__device__ __forceinline__ void block_tree(T* v, int tid, Op op) {
  __syncthreads();
  for (int o = kSurfThreads >> 1; o > 0; o >>= 1) {
    if (tid < o) v[tid] = op(v[tid], v[tid + o]);
    __syncthreads();
  }
}

struct SurfAcc {
  long long n[2], le[2];
  double sum[2], mx[2];
};

// sums the accumulators of the workgroup's threads; thread 0 then writes [n_p, le_p, n_g, le_g] and [sum_p, max_p, sum_g, max_g]
__device__ __forceinline__ void surf_acc_reduce(const SurfAcc& a, long long* cnt_out, double* val_out) {
  __shared__ long long sc[kSurfThreads];
  __shared__ double sd[kSurfThreads];
  const int tid = threadIdx.x;
  for (int q = 0; q < 4; ++q) {
    __syncthreads();
    sc[tid] = (q & 1) ? a.le[q >> 1] : a.n[q >> 1];
    block_tree(sc, tid, [](long long x, long long y) { return x + y; });
    if (tid == 0) cnt_out[q] = sc[0];
  }
  for (int q = 0; q < 4; ++q) {
    __syncthreads();
    sd[tid] = (q & 1) ? a.mx[q >> 1] : a.sum[q >> 1];
    if (q & 1)
      block_tree(sd, tid, [](double x, double y) { return fmax(x, y); });
    else
      block_tree(sd, tid, [](double x, double y) { return x + y; });
    if (tid == 0) val_out[q] = sd[0];
  }
}

__global__ void __launch_bounds__(kSurfThreads) surface_stats_kernel(const uint8_t* __restrict__ flags, const double* __restrict__ dg,
                                                                     const double* __restrict__ dp, int nj, int ni, SurfBox b, double tau,
                                                                     long long* __restrict__ pcnt, double* __restrict__ pval) {
  SurfAcc a = {{0, 0}, {0, 0}, {0.0, 0.0}, {0.0, 0.0}};
  const int bj = b.j1 - b.j0;
  const int64_t rows = (int64_t)(b.k1 - b.k0) * bj;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int k = b.k0 + (int)(row / bj), j = b.j0 + (int)(row % bj);
    const int64_t r0 = ((int64_t)k * nj + j) * ni;
    for (int i = b.i0 + threadIdx.x; i < b.i1; i += kSurfThreads) {
      const unsigned f = flags[r0 + i];
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (f & (1u << q)) {
          const double d = sqrt((q ? dp : dg)[r0 + i]);
          a.n[q] += 1;
          a.le[q] += d <= tau ? 1 : 0;
          a.sum[q] += d;
          a.mx[q] = fmax(a.mx[q], d);
        }
    }
  }
  surf_acc_reduce(a, pcnt + (size_t)blockIdx.x * 4, pval + (size_t)blockIdx.x * 4);
}

__global__ void __launch_bounds__(kSurfThreads) surface_stats_fold_kernel(const long long* __restrict__ pcnt, const double* __restrict__ pval, int nb,
                                                                          long long* __restrict__ counts, double* __restrict__ vals) {
  SurfAcc a = {{0, 0}, {0, 0}, {0.0, 0.0}, {0.0, 0.0}};
  for (int b = threadIdx.x; b < nb; b += kSurfThreads)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      a.n[q] += pcnt[(size_t)b * 4 + 2 * q];
      a.le[q] += pcnt[(size_t)b * 4 + 2 * q + 1];
      a.sum[q] += pval[(size_t)b * 4 + 2 * q];
      a.mx[q] = fmax(a.mx[q], pval[(size_t)b * 4 + 2 * q + 1]);
    }
  surf_acc_reduce(a, counts, vals);
}

// select state in the workspace: prefix[4], rank[4], then hist[pass][slot][bin]
struct SelState {
  unsigned long long prefix[kSelSlots];
  long long rank[kSelSlots];
};

__global__ void __launch_bounds__(kSurfThreads) surface_select_init_kernel(SelState* st, unsigned long long* hist, long long r0, long long r1, long long r2,
                                                                           long long r3) {
  const int e = blockIdx.x * kSurfThreads + threadIdx.x;
  if (e < kSelPasses * kSelSlots * kSelBins) hist[e] = 0;
  if (e < kSelSlots) {
    st->prefix[e] = 0;
    st->rank[e] = e == 0 ? r0 : e == 1 ? r1 : e == 2 ? r2 : r3;
  }
}

__global__ void __launch_bounds__(kSurfThreads) surface_select_hist_kernel(const uint8_t* __restrict__ flags, const double* __restrict__ dg,
                                                                           const double* __restrict__ dp, int nj, int ni, SurfBox b, int pass,
                                                                           const SelState* __restrict__ st, unsigned long long* __restrict__ hist) {
  __shared__ unsigned int h[kSelSlots * kSelBins];
  for (int e = threadIdx.x; e < kSelSlots * kSelBins; e += kSurfThreads) h[e] = 0;
  unsigned long long prefix[kSelSlots];
  bool live[kSelSlots];
#pragma unroll
  for (int s = 0; s < kSelSlots; ++s) {
    prefix[s] = st->prefix[s];
    live[s] = st->rank[s] >= 0;
  }
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const int bj = b.j1 - b.j0;
  const int64_t rows = (int64_t)(b.k1 - b.k0) * bj;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int k = b.k0 + (int)(row / bj), j = b.j0 + (int)(row % bj);
    const int64_t r0 = ((int64_t)k * nj + j) * ni;
    for (int i = b.i0 + threadIdx.x; i < b.i1; i += kSurfThreads) {
      const unsigned f = flags[r0 + i];
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (f & (1u << q)) {
          const unsigned long long u = (unsigned long long)__double_as_longlong((q ? dp : dg)[r0 + i]);
          const unsigned long long head = pass == 0 ? 0ull : u >> (shift + 8);
          const unsigned bin = (unsigned)(u >> shift) & 255u;
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const int s = 2 * q + r;
            if (live[s] && head == prefix[s]) atomicAdd(&h[s * kSelBins + bin], 1u);
          }
        }
    }
  }
  __syncthreads();
  unsigned long long* g = hist + (size_t)pass * kSelSlots * kSelBins;
  for (int e = threadIdx.x; e < kSelSlots * kSelBins; e += kSurfThreads)
    if (h[e]) atomicAdd(&g[e], (unsigned long long)h[e]);
}

// the bin that holds each rank: prefix <- prefix * 256 + bin, rank <- rank within the bin; after the last pass the prefix is the
// value's bit pattern and out[slot] its square root (NaN for a rank below 0: nothing was asked for)
__global__ void __launch_bounds__(64) surface_select_pick_kernel(SelState* st, const unsigned long long* __restrict__ hist, int pass, double* __restrict__ out) {
  const int s = threadIdx.x;
  if (s >= kSelSlots) return;
  const long long r = st->rank[s];
  if (r < 0) {
    if (pass == kSelPasses - 1) out[s] = __builtin_nan("");
    return;
  }
  const unsigned long long* h = hist + ((size_t)pass * kSelSlots + s) * kSelBins;
  unsigned long long cum = 0;
  int bin = 0;
  for (; bin < kSelBins - 1; ++bin) {  // a rank past the count ends in the last bin
    const unsigned long long c = h[bin];
    if (cum + c > (unsigned long long)r) break;
    cum += c;
  }
  const unsigned long long p = (st->prefix[s] << 8) | (unsigned long long)bin;
  st->prefix[s] = p;
  st->rank[s] = r - (long long)cum;
  if (pass == kSelPasses - 1) out[s] = sqrt(__longlong_as_double((long long)p));
}

int surf_check_shape(const char* what, int nk, int nj, int ni) {
  HCT_REQUIRE(nk >= 1 && nj >= 1 && ni >= 1 && std::max({nk, nj, ni}) <= kSurfMaxAxis, "%s: shape (%d, %d, %d): every axis must lie in [1, %d]", what, nk,
              nj, ni, kSurfMaxAxis);
  return 0;
}

int surf_check_box(const char* what, int nk, int nj, int ni, const SurfBox& b) {
  HCT_REQUIRE(0 <= b.k0 && b.k0 <= b.k1 && b.k1 <= nk && 0 <= b.j0 && b.j0 <= b.j1 && b.j1 <= nj && 0 <= b.i0 && b.i0 <= b.i1 && b.i1 <= ni,
              "%s: box [%d, %d) x [%d, %d) x [%d, %d) leaves the volume (%d, %d, %d)", what, b.k0, b.k1, b.j0, b.j1, b.i0, b.i1, nk, nj, ni);
  return 0;
}

bool box_empty(const SurfBox& b) { return b.k1 == b.k0 || b.j1 == b.j0 || b.i1 == b.i0; }

int scan_blocks(int64_t rows) { return (int)std::min<int64_t>(kSurfMaxBlocks, std::max<int64_t>(rows, 1)); }

int surf_check_ws(const char* what, const void* ws, size_t have, size_t need) {
  if (!ws || have < need || ((uintptr_t)ws % 8) != 0) {
    set_error("%s: workspace too small or not 8-byte aligned (%zu < %zu)", what, have, need);
    return HCT_E_WORKSPACE;
  }
  return 0;
}

}  // namespace
}  // namespace hct

using namespace hct;

extern "C" {

size_t hct_surface_edges_workspace_bytes(int nk, int nj, int ni) {
  if (nk < 1 || nj < 1 || ni < 1 || std::max({nk, nj, ni}) > kSurfMaxAxis) return 0;
  return (size_t)scan_blocks((int64_t)nk * nj) * 8 * sizeof(long long);
}

int hct_surface_edges(const int16_t* pred, const uint8_t* labels, int nk, int nj, int ni, int cls, uint8_t* flags, int64_t* out, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (int rc = surf_check_shape("hct_surface_edges", nk, nj, ni)) return rc;
  HCT_REQUIRE(pred && labels && flags && out, "hct_surface_edges: null pred, labels, flags or out");
  HCT_REQUIRE(cls >= 0 && cls <= 254, "hct_surface_edges: class %d outside [0, 254] (255 marks voxels that count nowhere)", cls);
  if (int rc = surf_check_ws("hct_surface_edges", workspace, workspace_bytes, hct_surface_edges_workspace_bytes(nk, nj, ni))) return rc;
  const int nb = scan_blocks((int64_t)nk * nj);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(surface_edges_kernel, dim3(nb), dim3(kSurfThreads), 0, s, pred, labels, nk, nj, ni, cls, flags, (long long*)workspace);
  hipLaunchKernelGGL(surface_edges_fold_kernel, dim3(1), dim3(kSurfThreads), 0, s, (const long long*)workspace, nb, (long long*)out);
  HCT_CHECK_LAUNCH("hct_surface_edges");
  return 0;
}

int hct_edt3d(const uint8_t* flags, int bit, int nk, int nj, int ni, int k0, int j0, int i0, int k1, int j1, int i1, double sk, double sj, double si,
              double* out, void* stream) {
  if (int rc = surf_check_shape("hct_edt3d", nk, nj, ni)) return rc;
  const SurfBox b = {k0, j0, i0, k1, j1, i1};
  if (int rc = surf_check_box("hct_edt3d", nk, nj, ni, b)) return rc;
  HCT_REQUIRE(flags && out, "hct_edt3d: null flags or out");
  HCT_REQUIRE(bit >= 1 && bit <= 255, "hct_edt3d: bit mask %d outside [1, 255]", bit);
  HCT_REQUIRE(std::isfinite(sk) && std::isfinite(sj) && std::isfinite(si) && sk > 0 && sj > 0 && si > 0, "hct_edt3d: spacing (%g, %g, %g) must be finite and > 0",
              sk, sj, si);
  const int bk = k1 - k0, bj = j1 - j0, bi = i1 - i0;
  if (std::max({bk, bj, bi}) > kEdtMaxLine) {
    set_error("hct_edt3d: box of (%d, %d, %d) voxels: a line of more than %d is not supported", bk, bj, bi, kEdtMaxLine);
    return HCT_E_UNSUPPORTED;
  }
  if (box_empty(b)) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int64_t row = ni, slab = (int64_t)nj * ni, base = ((int64_t)k0 * nj + j0) * ni + i0;
  // pass k (from the flags), pass j, pass i: (line length, line stride, tile neighbours' stride and count, outer stride and count)
  struct Pass {
    int L;
    int64_t ls, ws;
    int nw;
    int64_t os;
    int outer, fast_w;
    double s;
  } passes[3] = {{bk, slab, 1, bi, row, bj, 1, sk}, {bj, row, 1, bi, slab, bk, 1, sj}, {bi, 1, row, bj, slab, bk, 0, si}};
  for (int p = 0; p < 3; ++p) {
    const Pass& q = passes[p];
    const int W = edt_width(q.L), tiles_w = (q.nw + W - 1) / W;
    const size_t lds = (size_t)q.L * W * sizeof(double);  // at most 64 KiB
    hipLaunchKernelGGL(edt_pass_kernel, dim3((unsigned)((int64_t)q.outer * tiles_w)), dim3(kEdtThreads), lds, s, p == 0 ? flags : (const uint8_t*)nullptr, bit,
                       out, base, q.L, q.ls, W, q.ws, q.nw, tiles_w, q.os, q.fast_w, q.s);
  }
  HCT_CHECK_LAUNCH("hct_edt3d");
  return 0;
}

size_t hct_surface_stats_workspace_bytes(int nk, int nj, int ni) {
  if (nk < 1 || nj < 1 || ni < 1 || std::max({nk, nj, ni}) > kSurfMaxAxis) return 0;
  return (size_t)scan_blocks((int64_t)nk * nj) * 4 * (sizeof(long long) + sizeof(double));
}

int hct_surface_stats(const uint8_t* flags, const double* dist_g, const double* dist_p, int nk, int nj, int ni, int k0, int j0, int i0, int k1, int j1,
                      int i1, double tau, int64_t* counts, double* vals, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = surf_check_shape("hct_surface_stats", nk, nj, ni)) return rc;
  const SurfBox b = {k0, j0, i0, k1, j1, i1};
  if (int rc = surf_check_box("hct_surface_stats", nk, nj, ni, b)) return rc;
  HCT_REQUIRE(flags && dist_g && dist_p && counts && vals, "hct_surface_stats: null flags, distance field, counts or vals");
  HCT_REQUIRE(tau >= 0 && !std::isnan(tau), "hct_surface_stats: tolerance %g must be >= 0", tau);
  if (int rc = surf_check_ws("hct_surface_stats", workspace, workspace_bytes, hct_surface_stats_workspace_bytes(nk, nj, ni))) return rc;
  const int64_t rows = box_empty(b) ? 0 : (int64_t)(k1 - k0) * (j1 - j0);
  const int nb = scan_blocks(rows);
  long long* pcnt = (long long*)workspace;
  double* pval = (double*)(pcnt + (size_t)nb * 4);
  hipStream_t s = (hipStream_t)stream;
  const SurfBox run = rows ? b : SurfBox{0, 0, 0, 0, 0, 0};
  hipLaunchKernelGGL(surface_stats_kernel, dim3(nb), dim3(kSurfThreads), 0, s, flags, dist_g, dist_p, nj, ni, run, tau, pcnt, pval);
  hipLaunchKernelGGL(surface_stats_fold_kernel, dim3(1), dim3(kSurfThreads), 0, s, (const long long*)pcnt, (const double*)pval, nb, (long long*)counts, vals);
  HCT_CHECK_LAUNCH("hct_surface_stats");
  return 0;
}

size_t hct_surface_select_workspace_bytes(void) { return sizeof(SelState) + (size_t)kSelPasses * kSelSlots * kSelBins * sizeof(unsigned long long); }

int hct_surface_select(const uint8_t* flags, const double* dist_g, const double* dist_p, int nk, int nj, int ni, int k0, int j0, int i0, int k1, int j1,
                       int i1, int64_t rank_p_lo, int64_t rank_p_hi, int64_t rank_g_lo, int64_t rank_g_hi, double* out, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (int rc = surf_check_shape("hct_surface_select", nk, nj, ni)) return rc;
  const SurfBox b = {k0, j0, i0, k1, j1, i1};
  if (int rc = surf_check_box("hct_surface_select", nk, nj, ni, b)) return rc;
  HCT_REQUIRE(flags && dist_g && dist_p && out, "hct_surface_select: null flags, distance field or out");
  if (int rc = surf_check_ws("hct_surface_select", workspace, workspace_bytes, hct_surface_select_workspace_bytes())) return rc;
  const int64_t rows = box_empty(b) ? 0 : (int64_t)(k1 - k0) * (j1 - j0);
  const int nb = scan_blocks(rows);
  const SurfBox run = rows ? b : SurfBox{0, 0, 0, 0, 0, 0};
  SelState* st = (SelState*)workspace;
  unsigned long long* hist = (unsigned long long*)(st + 1);
  hipStream_t s = (hipStream_t)stream;
  const int cells = kSelPasses * kSelSlots * kSelBins;
  hipLaunchKernelGGL(surface_select_init_kernel, dim3((cells + kSurfThreads - 1) / kSurfThreads), dim3(kSurfThreads), 0, s, st, hist, (long long)rank_p_lo,
                     (long long)rank_p_hi, (long long)rank_g_lo, (long long)rank_g_hi);
  for (int pass = 0; pass < kSelPasses; ++pass) {
    hipLaunchKernelGGL(surface_select_hist_kernel, dim3(nb), dim3(kSurfThreads), 0, s, flags, dist_g, dist_p, nj, ni, run, pass, (const SelState*)st, hist);
    hipLaunchKernelGGL(surface_select_pick_kernel, dim3(1), dim3(64), 0, s, st, (const unsigned long long*)hist, pass, out);
  }
  HCT_CHECK_LAUNCH("hct_surface_select");
  return 0;
}

}  // extern "C"
