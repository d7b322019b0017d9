// How a GEMM launch is planned: which kernel, which epilogue instance, tile height, grid, stream-K remainder, split-K and workspace
// layout, as pure functions of (hct_gemm_args, CU count, tuning).  Plain C++17 with no HIP header, so the same code that gemm.hip
// launches from is compiled and swept on the CPU (tests/host/gemm_plan_sweep.cpp, hct_gemm_describe).  plan_gemm allocates nothing;
// only the grouped-wgrad tile ordering at the end uses std::vector.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/headct_hip.h"

#ifdef __HIPCC__
#define HCT_HOST_DEVICE __host__ __device__ inline __attribute__((always_inline))
#else
#define HCT_HOST_DEVICE inline
#endif

namespace hct {

// epilogue instances of the tuned NT kernels (gemm.hip, "specialised epilogues")
enum { EPI_GENERIC = 0, EPI_PLAIN_BF16 = 1, EPI_RES_F32 = 2, EPI_GELU_BF16 = 3, EPI_DGELU_BF16 = 4, EPI_PLAIN_F32 = 5,
       EPI_DGELU_CS = 6 /* DGELU + fused column sums of the output (own instance: costs registers in the epilogue) */ };

// stream-K region of the NT workspace (its LAST kSkBytes): [flags: one word per workgroup | error word] then one 256-KiB slab of
// raw fp32 accumulators per workgroup
constexpr int kSkMaxWgs = 256;
constexpr size_t kSkHeadBytes = 4096, kSkSlabBytes = 262144;
constexpr size_t kSkBytes = kSkHeadBytes + (size_t)kSkMaxWgs * kSkSlabBytes;
constexpr int kTnMaxFollowers = 1024;  // follower pieces (= slabs) of the grouped wgrad kernel's remainder

struct GemmTuning {        // hct_debug_set_gemm_variant
  int nt_variant = 0;      // 0 auto; 128 / 256 force one NT kernel (tests cover both); 128 also keeps wgrads off the 256x256 TN kernel
  bool mt3 = true;         // (-14 / -15: on / off) 192-row tiles for single-round plain / +residual shapes
  bool sk_drop = false;    // (-8 / -9) testing: stream-K followers publish a wrong sequence number -> every owner times out
  int sk_min_k = 512;      // (-1000 - k) stream-K of the NT remainder round only for K >= this; k > any K switches it off
  int sk_gain_pairs = 20;  // (-100 - n) ... and only where it saves at least n stage pairs per CU; a huge value = whole tiles only
  int walk_width = 0;      // (-20 - w) tile walk of the NT256 kernel: 0 = n fastest over all of N (the default), 1 .. 78 = bands of w column tiles, 79 = nt_walk_width's bands
};

enum { GEMM_GENERIC = HCT_GEMM_GENERIC, GEMM_NT128 = HCT_GEMM_NT128, GEMM_NT256 = HCT_GEMM_NT256, GEMM_TN128 = HCT_GEMM_TN128,
       GEMM_TN256 = HCT_GEMM_TN256 };
typedef hct_gemm_plan_info GemmPlan;  // (one struct: what hct_gemm launches from is what hct_gemm_describe reports)
constexpr size_t kNoOffset = (size_t)-1;
constexpr size_t kUnlimited = (size_t)-1;

inline bool aligned_to(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p % a) == 0; }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int ceil_div(int v, int d) { return (v + d - 1) / d; }

inline bool epilogue_vec_ok(const hct_gemm_args* a) {
  auto ok = [](const void* p, int dt, int64_t ld) { return p == nullptr || (ld % 4 == 0 && aligned_to(p, dt == HCT_BF16 ? 8 : 16)); };
  return a->N % 4 == 0 && ok(a->C, a->c_dtype, a->ldc) && ok(a->C2, a->c2_dtype, a->ldc2) && ok(a->aux, a->aux_dtype, a->ldaux) &&
         ok(a->residual, HCT_F32, a->ldr) && aligned_to(a->bias, 16);
}

enum Path { PATH_GENERIC = 0, PATH_NT = 1, PATH_TN = 2 };

inline Path choose_path(const hct_gemm_args* a) {
  if (a->force_generic || a->a_dtype != HCT_BF16 || a->b_dtype != HCT_BF16) return PATH_GENERIC;
  if (!epilogue_vec_ok(a)) return PATH_GENERIC;
  if (!aligned_to(a->A, 16) || !aligned_to(a->B, 16) || a->lda % 8 || a->ldb % 8) return PATH_GENERIC;
  if (a->transA == 0 && a->transB == 1 && a->K % 64 == 0 && a->N % 16 == 0 && a->lda * 2 * 128 < (1ll << 31) && a->ldb * 2 * 128 < (1ll << 31))
    return PATH_NT;
  if (a->transA == 1 && a->transB == 0 && a->M % 16 == 0 && a->N % 16 == 0 && a->act == HCT_ACT_NONE && !a->bias && !a->residual &&
      (int64_t)a->K * a->lda * 2 < (1ll << 40))
    return PATH_TN;
  return PATH_GENERIC;
}

inline int epilogue_mode(const hct_gemm_args* a) {
  if (a->C2) return EPI_GENERIC;
  const bool small = a->ldc * 256 < (1ll << 28) && a->ldr * 256 < (1ll << 28) && a->ldaux * 256 < (1ll << 28);
  if (!small) return EPI_GENERIC;
  // bf16 outputs are stored 8 columns (16 B) per lane
  auto wide_ok = [](const void* p, int64_t ld) { return p == nullptr || (ld % 8 == 0 && aligned_to(p, 16)); };
  if (a->c_dtype == HCT_BF16 && !(a->N % 8 == 0 && wide_ok(a->C, a->ldc) && wide_ok(a->aux, a->ldaux))) return EPI_GENERIC;
  if (a->act == HCT_ACT_NONE && !a->residual && a->c_dtype == HCT_BF16) return EPI_PLAIN_BF16;
  if (a->act == HCT_ACT_NONE && a->residual && a->c_dtype == HCT_F32) return EPI_RES_F32;
  const bool is_gelu = a->act == HCT_ACT_GELU || a->act == HCT_ACT_GELU_D, is_dgelu = a->act == HCT_ACT_DGELU || a->act == HCT_ACT_MULAUX;
  if (is_gelu && !a->residual && a->c_dtype == HCT_BF16 && a->aux && a->aux_dtype == HCT_BF16) return EPI_GELU_BF16;
  if (is_dgelu && !a->residual && a->c_dtype == HCT_BF16 && a->aux_dtype == HCT_BF16) return EPI_DGELU_BF16;
  return EPI_GENERIC;
}

// Stream-K for the remainder round of the persistent 256x256 NT kernel.  What it saves is the idle share of the last round, in
// stage pairs per CU; what it costs is one 256-KiB slab out and one or two in per workgroup, a second pipeline fill, and the
// clock / bandwidth head-room that the idle CUs were leaving to the busy ones.  Measured inside the training step
// (scripts/ab_step.py sk20 / sk16 / skoff): a threshold of 20 pairs -- the decoder's K = 3072 GEMMs with 651 tiles, 22 pairs
// saved -- is 0.23 ms per step faster than whole tiles; 16 (adds the encoder's 165-tile K = 3072 and the decoder's K = 2304
// GEMMs) is 0.10 ms slower, 8 is 0.3 ms slower.
inline bool nt_stream_k(int K, int tiles256, int G, const GemmTuning& t, int& sk_tiles, int& sk_wgs) {
  sk_tiles = sk_wgs = 0;
  const int P = K / 64;
  if (G > kSkMaxWgs || K < t.sk_min_k || P < 8 || P > 1023) return false;
  const int rem = tiles256 % G;  // (< 256: fits the packed item's tile field)
  if (rem == 0 || (int64_t)(G - rem) * P < (int64_t)t.sk_gain_pairs * G) return false;
  // per XCD (grid / 8 workgroups, ceil(rem / 8) tiles at most): every K range at least four pairs long and shorter than a tile
  const int gx = G / 8, nxmax = (rem + 7) / 8;
  if (G % 8 || (int64_t)nxmax * P > (int64_t)gx * (P - 1)) return false;
  sk_tiles = rem;
  // workgroups per XCD that may take a K range: one per four stage pairs of the XCD's share of the remainder tiles, ceil(rem / 8)
  // of them (rem / 8 gave ONE workgroup per XCD for rem < 8: a stream-K launch that shared nothing)
  sk_wgs = (int)std::min<int64_t>(gx, std::max<int64_t>(1, (int64_t)nxmax * P / 4));
  return true;
}

// The stream-K work items of workgroup `wg` (the device side of nt_stream_k; gemm_bf16_nt256_kernel<MODE, SK = true> explains the
// scheme).  XCD x = wg & 7 shares out its own slice of the sk_tiles remainder tiles over its own workgroups j = wg >> 3: in units
// of stage pairs (P per tile) the slice is cut into contiguous ranges, and a range is split at the tile boundary into at most one
// piece that starts inside a tile (follower) and one that starts a tile (owner).  An item is one packed word:
//   tile id [0,8) | first pair [8,18) | pairs [18,28) | followers to collect [28,31) | bit 31: owner present
// `first` is what the workgroup computes first (its follower piece, else its owner piece), `owner` an owner piece that comes
// second; 0 = none.
HCT_HOST_DEVICE void stream_k_items(unsigned wg, int sk_tiles, int sk_wgs, int P, uint32_t& first, uint32_t& owner) {
  first = owner = 0;
  const int x = wg & 7, j = wg >> 3;
  const int t0 = (x * sk_tiles) >> 3, nx = (((x + 1) * sk_tiles) >> 3) - t0;  // this XCD's tiles [t0, t0 + nx)
  const int wx = sk_wgs < nx * 4 ? sk_wgs : nx * 4;                           // its workgroups that take a K range (<= 4 per tile)
  if (j < wx) {
    auto sk_bound = [&](int c) -> int {
      if (c >= wx) return nx * P;
      const int v = (int)(((int64_t)c * nx * P) / wx);
      const int r = v % P;  // no piece shorter than two pairs (the pipeline needs four stages): snap to the tile boundary
      return r == 1 ? v - 1 : (r == P - 1 ? v + 1 : v);
    };
    int b = sk_bound(j);
    const int en = sk_bound(j + 1);
    int t = b / P;
    const int off = b - t * P;
    if (off) {
      const int pe = en < (t + 1) * P ? en : (t + 1) * P;
      first = (uint32_t)(t0 + t) | ((uint32_t)off << 8) | ((uint32_t)(pe - b) << 18);
      b = pe;
      ++t;
    }
    if (b < en) {  // b == t * P: this workgroup starts tile t; the host keeps every range shorter than a tile
      const int tend = (t + 1) * P;
      uint32_t nf = 0;
      for (int c2 = j + 1; c2 < wx && sk_bound(c2) < tend; ++c2) ++nf;
      owner = (uint32_t)(t0 + t) | ((uint32_t)((en < tend ? en : tend) - b) << 18) | (nf << 28) | 0x80000000u;  // (bit 31: present)
    }
    if (!first) { first = owner; owner = 0; }
  }
}

// ---- tile walk of the persistent NT kernel ---------------------------------------------------------------------------------------
// The 32 CUs of an XCD work on 32 consecutive walk positions at a time (gemm_bf16_nt256_kernel, dp_id) and go on to the next 32
// a tile time later.  With n fastest over all of N those 32 tiles are min(ntn, 32) weight panels x a few row panels, one panel =
// 256 rows x K bf16: for N = 3072, K = 768 that is 12 x 384 KiB of weights alone, more than the 4-MiB L2 of an XCD together with
// the round's row panels, so every round fetches the weights again.  The walk can therefore be cut into BANDS of w column tiles: n
// fastest inside a band, then down M, then the next band.  An XCD's slice of the walk is contiguous, so it keeps its w weight
// panels over consecutive rounds while the row panels stream past; every band reads A again, which is why the bands are as wide
// as the budget allows and all about equally wide.  (Not the default: GemmTuning::walk_width, plan_gemm.)
constexpr size_t kXcdL2Bytes = 4u << 20;
constexpr size_t kWalkWeightBudget = kXcdL2Bytes / 2;  // the window's weight panels: the other half is left to a round's row panels
constexpr int kXcdWindow = 32;                         // CUs per XCD = tiles in flight per XCD

// Column tiles per band; ntn = the whole of N in one band (today's order).  Launches of one round keep today's order: nothing
// is reused from round to round.  Panels too long for two of them to fit the budget (K = 3072: 1.5 MiB each) do as well: a
// band of one would read A ntn times.
inline int nt_walk_width(int ntn, int K, int tiles, int G) {
  if (tiles <= G || ntn < 2) return ntn;
  const size_t panel = (size_t)256 * K * 2;
  const int wmax = (int)std::min<size_t>(kWalkWeightBudget / panel, kXcdWindow);
  if (wmax >= ntn || wmax < 2) return ntn;
  const int bands = ceil_div(ntn, wmax);
  return ceil_div(ntn, bands);
}

// Workgroups are dealt to the XCDs round-robin (XCD = blockIdx & 7), and a workgroup's virtual block ids vb = blockIdx, + grid, ...
// (grid a multiple of 8, or a single round) stay on its XCD: XCD x gets the x-th of eight contiguous slices of the nwg walk
// positions, the first nwg % 8 slices one longer.
HCT_HOST_DEVICE int nt_xcd_pos(int vb, int nwg) {
  const int xcd = vb & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (vb >> 3);
}

// Whole-tile walk position `pos` in [0, ntiles - sk_tiles) -> tile id in [sk_tiles, ntiles) (id = row tile * ntn + column tile), a
// bijection for every w.  The stream-K remainder tiles keep the ids [0, sk_tiles): which tiles are shared out, and with them the
// summation order of every output, does not depend on the walk.  The row of tiles that the remainder ends in is walked first, n
// fastest; the full rows below it in bands of w.
HCT_HOST_DEVICE int nt_walk_id(int pos, int ntiles, int ntn, int sk_tiles, int w) {
  if (w <= 0 || w >= ntn) return sk_tiles + pos;
  const int r0 = (sk_tiles + ntn - 1) / ntn;
  const int lead = (r0 * ntn < ntiles ? r0 * ntn : ntiles) - sk_tiles;
  if (pos < lead) return sk_tiles + pos;
  const int p = pos - lead, band = (ntiles / ntn - r0) * w;
  const int b = p / band, r = p - b * band;
  const int wb = ntn - b * w < w ? ntn - b * w : w;
  const int tr = r / wb;
  return (r0 + tr) * ntn + b * w + (r - tr * wb);
}

inline bool tn256_ok(const hct_gemm_args* a, const GemmTuning& t) {
  return t.nt_variant != 128 && a->c_dtype == HCT_F32 && !a->C2 && a->ldc % 4 == 0 && a->ldc * 256 < (1ll << 28) &&
         a->lda * 2 * 64 < (1ll << 31) && a->ldb * 2 * 64 < (1ll << 31);
}

inline void tn256_split(const hct_gemm_args* a, int G, int& splits, int& r_chunk) {
  const int tiles = std::max(1, ceil_div(a->M, 256) * ceil_div(a->N, 256));
  int s = std::max(1, G / tiles);
  int per = (a->K + s - 1) / s;
  per = std::max(128, (per + 63) / 64 * 64);  // even stage count >= 4
  // keep a split's operand span inside the 32-bit buffer offset range
  while ((int64_t)per * std::max(a->lda, a->ldb) * 2 >= (1ll << 31)) per = std::max(128, per / 2 / 64 * 64);
  r_chunk = per;
  splits = (a->K + per - 1) / per;
}

inline void tn_split(const hct_gemm_args* a, int& splits, int& r_chunk) {
  const int tiles = std::max(1, ceil_div(a->M, 128) * ceil_div(a->N, 128));
  const int steps = (a->K + 63) / 64;
  int s = (1024 + tiles - 1) / tiles;
  if (s > steps / 4) s = steps / 4;
  if (s < 1) s = 1;
  int per = (steps + s - 1) / s;
  r_chunk = per * 64;
  splits = (a->K + r_chunk - 1) / r_chunk;
}

// hct_colsum (elementwise.hip): row chunks of its partial sums
inline int colsum_chunks(int rows, int cols) {
  const int colblk = (cols + 255) / 256;
  int chunks = (1024 + colblk - 1) / colblk;
  if (chunks > (rows + 15) / 16) chunks = (rows + 15) / 16;
  return chunks < 1 ? 1 : chunks;
}
// column sums of C: the larger of the fused form's per-(tile-row, wave-row) partials and the separate pass's (hct_colsum)
inline size_t colsum_ws(const hct_gemm_args* a) {
  if (!a->colsum_out) return 0;
  const size_t fused = (size_t)ceil_div(a->M, 256) * 4 * a->N * sizeof(float);
  return std::max(fused, (size_t)colsum_chunks(a->M, a->N) * a->N * sizeof(float));
}

// Workspace of an NT / generic launch: the column-sum partials (if asked for) at its head; the stream-K region is its LAST kSkBytes,
// from a 256-byte boundary, and is there only if the workspace has room for both.  `head_bytes` = what the front part may use.
struct WsLayout { size_t head_bytes, stream_k_offset; };
inline WsLayout ws_layout(size_t colsum_bytes, size_t workspace_bytes) {
  if (workspace_bytes < align256(colsum_bytes) + kSkBytes) return WsLayout{workspace_bytes, kNoOffset};
  const size_t off = (workspace_bytes - kSkBytes) & ~(size_t)255;
  return WsLayout{off, off};
}

// The whole decision for one hct_gemm call on `num_cus` CUs.  `available` = bytes of workspace the caller passes (0: none;
// kUnlimited: whatever the plan asks for): a workspace too small for the stream-K region gets whole tiles.  plan.workspace_bytes
// is the request (hct_gemm_workspace_bytes) and does not depend on `available`.
//   tiles / grid: NT256 tiles of 256 (or 192) x 256 and workgroups; NT128 / TN128 128 x 128 tiles (TN128: grid.y = splits);
//   TN256 tiles x splits and workgroups; generic 64 x 64 tiles.
inline GemmPlan plan_gemm(const hct_gemm_args* a, int num_cus, const GemmTuning& t, size_t available) {
  GemmPlan p;
  memset(&p, 0, sizeof(p));
  p.row_tiles_per_wave = 4;
  p.splits = 1;
  p.stream_k_offset = kNoOffset;
  p.colsum_bytes = colsum_ws(a);
  p.workspace_bytes = p.colsum_bytes;
  const Path path = choose_path(a);
  const int G = num_cus;
  if (path == PATH_NT && a->K >= 128 && (t.nt_variant == 0 || t.nt_variant == 256)) {  // (K % 64 == 0: choose_path)
    p.kernel = GEMM_NT256;
    p.epilogue_mode = epilogue_mode(a);
    // (any M: rows past M are masked out of the sums, and every (row tile, wave) partial row is written -- zeros where a
    //  wave's 64 rows lie wholly past M -- so the fixed-order fold over ceil(M / 256) * 4 rows sees no stale data)
    p.fuse_colsum = a->colsum_out && p.epilogue_mode == EPI_DGELU_BF16;
    const int tiles256 = ceil_div(a->M, 256) * ceil_div(a->N, 256);
    p.tiles = tiles256;
    const int ntn = ceil_div(a->N, 256);
    // (no bands by default: inside the training step the bands measured no gain; the hook keeps them testable)
    auto walk = [&](int tiles) { return t.walk_width == 0 ? ntn : t.walk_width >= 79 ? nt_walk_width(ntn, a->K, tiles, G) : std::min(t.walk_width, ntn); };
    p.walk_width = walk(tiles256);
    // stream-K for the remainder round: asked for only where the remainder round of THIS shape would be shared out on this CU count
    // (a caller that allocates per call -- the DINO head's Linears -- then neither reserves 64 MiB nor resets flags for shapes
    // that never split), used only if the workspace has the region
    int sk_tiles = 0, sk_wgs = 0;
    if (nt_stream_k(a->K, tiles256, G, t, sk_tiles, sk_wgs)) {
      p.workspace_bytes = align256(p.colsum_bytes) + kSkBytes;
      p.stream_k_offset = ws_layout(p.colsum_bytes, available == kUnlimited ? p.workspace_bytes : available).stream_k_offset;
    }
    if (p.stream_k_offset != kNoOffset) {
      p.sk_tiles = sk_tiles;
      p.sk_wgs = sk_wgs;
      p.grid = G;
      return p;
    }
    // Whole-tile launches: R = ceil(tiles / CUs) rounds take the same time on ceil(tiles / R) workgroups as on all CUs -- the last
    // round is then full and the CUs left out idle for the whole launch instead of for its last round only, which leaves their
    // share of the power budget to the others
    p.grid = std::min(tiles256, G);
    if (tiles256 > G) {
      const int rounds = ceil_div(tiles256, G);
      p.grid = std::min(G, (ceil_div(tiles256, rounds) + 7) / 8 * 8);  // (a multiple of 8: the tile walk deals ids per XCD)
    }
    // 192-row tiles for the plain / +residual shapes whose 256-row tiles fill less than one round of CUs while 192-row tiles still
    // fit one (the encoder's M = 14 080, N = 768 products: 165 -> 222 tiles, each 3/4 of the work)
    const int tiles192 = ceil_div(a->M, 192) * ceil_div(a->N, 256);
    if (t.mt3 && (p.epilogue_mode == EPI_PLAIN_BF16 || p.epilogue_mode == EPI_RES_F32) && tiles256 < G && tiles192 <= G && tiles192 > tiles256 &&
        a->M >= 192) {
      p.row_tiles_per_wave = 3;
      p.tiles = p.grid = tiles192;
      p.walk_width = walk(tiles192);
    }
    return p;
  }
  if (path == PATH_NT) {
    p.kernel = GEMM_NT128;
    p.tiles = p.grid = ceil_div(a->M, 128) * ceil_div(a->N, 128);
    return p;
  }
  if (path == PATH_TN) {
    if (tn256_ok(a, t)) {
      p.kernel = GEMM_TN256;
      tn256_split(a, G, p.splits, p.r_chunk);
      p.tiles = ceil_div(a->M, 256) * ceil_div(a->N, 256) * p.splits;
      p.grid = std::min(p.tiles, G);
    } else {
      p.kernel = GEMM_TN128;
      tn_split(a, p.splits, p.r_chunk);
      p.tiles = p.grid = ceil_div(a->M, 128) * ceil_div(a->N, 128);
    }
    p.slab_bytes = p.splits > 1 ? (size_t)p.splits * a->M * a->N * sizeof(float) : 0;
    p.workspace_bytes = p.slab_bytes;  // (colsum_out is refused on this path)
    return p;
  }
  p.kernel = GEMM_GENERIC;
  p.tiles = p.grid = ceil_div(a->N, 64) * ceil_div(a->M, 64);
  return p;
}

// ---- grouped wgrad (gemm_bf16_tn_group_kernel): which products may join, and the order of their tiles -------------------------------
inline bool tn_group_ok(const hct_gemm_args* a) {  // (quiet form for the model driver: falls back to the split-K launch otherwise)
  return a->transA == 1 && a->transB == 0 && a->a_dtype == HCT_BF16 && a->b_dtype == HCT_BF16 && a->c_dtype == HCT_F32 && !a->bias &&
         !a->residual && a->act == HCT_ACT_NONE && !a->aux && !a->C2 && !a->colsum_out && a->M > 0 && a->N > 0 && a->K > 0 && a->M % 16 == 0 &&
         a->N % 16 == 0 && a->lda % 8 == 0 && a->ldb % 8 == 0 && a->ldc % 4 == 0 && aligned_to(a->A, 16) && aligned_to(a->B, 16) &&
         aligned_to(a->C, 16) && a->A && a->B && a->C && a->ldc * 256 < (1ll << 28) && (int64_t)a->K * a->lda * 2 < 0xFFFFFFF0ll &&
         (int64_t)a->K * a->ldb * 2 < 0xFFFFFFF0ll && a->lda < (1 << 24) && a->ldb < (1 << 24);
}

template <typename BF16>  // (the device's bf16 type: this header names no device type)
struct TnJobT {           // 80 bytes, device copy written by tn_group_table_kernel
  const BF16* A; const BF16* B; float* C;
  int M, N, R, lda, ldb, ldc;
  int tile0, ntiles, ntn, nk;  // (tile0 unused by the kernel), tiles, column tiles, stages per tile (R / 32 rounded up to a multiple of 4)
  float alpha; int pad[3];
};
struct TnSeg { int job, tile_first, count, gtile0; };  // tiles [tile_first, tile_first + count) of `job` have the ids gtile0 ..
inline int tn_group_seg_capacity(int n) { return 16 * n + 64; }

template <typename BF16>
inline TnJobT<BF16> tn_group_job(const hct_gemm_args* a, int tile0) {
  TnJobT<BF16> j;
  memset(&j, 0, sizeof(j));
  j.A = (const BF16*)a->A; j.B = (const BF16*)a->B; j.C = (float*)a->C;
  j.M = a->M; j.N = a->N; j.R = a->K; j.lda = (int)a->lda; j.ldb = (int)a->ldb; j.ldc = (int)a->ldc;
  j.ntn = ceil_div(a->N, 256);
  j.ntiles = ceil_div(a->M, 256) * j.ntn;
  j.tile0 = tile0;
  j.nk = std::max(4, ((a->K + 31) / 32 + 3) / 4 * 4);
  j.alpha = a->alpha;
  return j;
}

// Tile order of a grouped launch.  Jobs by falling reduction length (stable), so that the whole-tile rounds are homogeneous and the
// shortest products end up in the remainder; inside a class of equal length the tiles are dealt in windows of 32 ids (= what the
// 32 workgroups of an XCD work on at a time): whole chunks of 32 tiles of ONE product while there are any, the left-overs packed
// largest-first into the windows that remain (a left-over is cut only where nothing fits).
template <typename Job>
inline std::vector<TnSeg> tn_group_segments(const std::vector<Job>& jobs) {
  std::vector<int> order(jobs.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return jobs[x].nk > jobs[y].nk; });
  std::vector<TnSeg> segs;
  int gid = 0;
  auto emit = [&](int job, int first, int count) {
    if (!segs.empty() && segs.back().job == job && segs.back().tile_first + segs.back().count == first) segs.back().count += count;
    else segs.push_back(TnSeg{job, first, count, gid});
    gid += count;
  };
  size_t i = 0;
  while (i < order.size()) {
    size_t e = i;
    while (e < order.size() && jobs[order[e]].nk == jobs[order[i]].nk) ++e;
    struct Item { int job, first, count; };
    std::vector<Item> full, rest;  // chunks of 32, left-overs (< 32)
    for (size_t k = i; k < e; ++k) {
      const int j = order[k], nt = jobs[j].ntiles;
      for (int c = 0; c + 32 <= nt; c += 32) full.push_back(Item{j, c, 32});
      if (nt % 32) rest.push_back(Item{j, nt / 32 * 32, nt % 32});
    }
    std::stable_sort(rest.begin(), rest.end(), [](const Item& x, const Item& y) { return x.count > y.count; });
    size_t fi = 0;
    while (fi < full.size() || !rest.empty()) {
      const int room = 32 - gid % 32;
      if (room == 32 && fi < full.size()) { emit(full[fi].job, full[fi].first, 32); ++fi; continue; }
      // the largest left-over that fits the window; none: a piece of the largest one (or of a whole chunk) closes the window
      size_t pick = rest.size();
      for (size_t k = 0; k < rest.size(); ++k)
        if (rest[k].count <= room) { pick = k; break; }
      if (pick < rest.size()) {
        emit(rest[pick].job, rest[pick].first, rest[pick].count);
        rest.erase(rest.begin() + pick);
      } else if (!rest.empty()) {
        emit(rest[0].job, rest[0].first, room);
        rest[0].first += room; rest[0].count -= room;
        std::stable_sort(rest.begin(), rest.end(), [](const Item& x, const Item& y) { return x.count > y.count; });
      } else {  // only whole chunks left and the window is open: cut one
        Item it = full[fi++];
        emit(it.job, it.first, room);
        rest.push_back(Item{it.job, it.first + room, 32 - room});
      }
    }
    i = e;
  }
  return segs;
}

// shortest reduction (in stages) among the remainder tiles of a grouped launch, i.e. the tile ids >= first_id
template <typename Job>
inline int tn_group_min_nk(const std::vector<Job>& jobs, const std::vector<TnSeg>& segs, int first_id) {
  int min_nk = 1 << 30;
  for (const TnSeg& sg : segs)
    if (sg.gtile0 + sg.count > first_id) min_nk = std::min(min_nk, jobs[sg.job].nk);
  return min_nk;
}

// splits of the remainder tiles: least (rounds of pieces) / splits, a small price per split for the fix-up; every piece at least
// 4 stages, at most kTnMaxFollowers follower pieces
inline int tn_group_splits(int Rm, int G, int min_nk) {
  if (Rm <= 0) return 1;
  int best = 1;
  double best_cost = 1e30;
  for (int sp = 1; sp <= 16; ++sp) {
    if (sp > 1 && ((int64_t)(sp - 1) * Rm > kTnMaxFollowers || min_nk / 4 < sp * 4)) break;  // (pieces of at least 16 stages)
    const double cost = (double)(((int64_t)Rm * sp + G - 1) / G) / sp + 0.004 * sp;
    if (cost < best_cost - 1e-12) { best_cost = cost; best = sp; }
  }
  return best;
}

}  // namespace hct
