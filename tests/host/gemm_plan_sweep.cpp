// Host sweep of csrc/gemm_plan.h (plain C++, no HIP): built with -fsanitize=address,undefined and run as a child process by
// tests/test_gemm_plan_host_cpu.py.  Exit status 0 and a last line "ok ..." = every check held.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../../headct_foundation_amd/csrc/gemm_plan.h"

using namespace hct;

#define CHECK(cond, ...)                               \
  do {                                                 \
    if (!(cond)) {                                     \
      fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                    \
      fprintf(stderr, "\n");                           \
      exit(1);                                         \
    }                                                  \
  } while (0)

typedef TnJobT<uint16_t> Job;   // (any 2-byte element type: the ordering reads ntiles and nk only)
struct Shape { int R, M, N; };  // one wgrad: dW[M, N] over R token rows

static void* const kPtr = (void*)256;  // an aligned address: nothing is dereferenced

static hct_gemm_args wgrad(const Shape& s) {
  hct_gemm_args a;
  memset(&a, 0, sizeof(a));
  a.M = s.M; a.N = s.N; a.K = s.R;
  a.A = kPtr; a.a_dtype = HCT_BF16; a.lda = s.M; a.transA = 1;
  a.B = kPtr; a.b_dtype = HCT_BF16; a.ldb = s.N; a.transB = 0;
  a.C = kPtr; a.c_dtype = HCT_F32; a.ldc = s.N;
  a.alpha = 1.0f;
  return a;
}

static long g_lists = 0, g_unsplit_short = 0;

static void check_group(const std::vector<Shape>& shapes, const char* what) {
  const int n = (int)shapes.size();
  std::vector<Job> jobs(n);
  int T = 0;
  for (int i = 0; i < n; ++i) {
    const hct_gemm_args a = wgrad(shapes[i]);
    CHECK(tn_group_ok(&a), "%s: job %d (R %d, M %d, N %d)", what, i, shapes[i].R, shapes[i].M, shapes[i].N);
    jobs[i] = tn_group_job<uint16_t>(&a, T);
    CHECK(jobs[i].ntiles == ceil_div(shapes[i].M, 256) * ceil_div(shapes[i].N, 256) && jobs[i].nk % 4 == 0 && jobs[i].nk * 32 >= shapes[i].R,
          "%s: job %d", what, i);
    T += jobs[i].ntiles;
  }
  const std::vector<TnSeg> segs = tn_group_segments(jobs);
  CHECK((int)segs.size() <= tn_group_seg_capacity(n), "%s: %zu segments for %d jobs", what, segs.size(), n);
  // every tile of every job exactly once, ids contiguous
  std::vector<std::vector<int>> seen(n);
  for (int i = 0; i < n; ++i) seen[i].assign(jobs[i].ntiles, 0);
  int gid = 0;
  for (const TnSeg& sg : segs) {
    CHECK(sg.job >= 0 && sg.job < n && sg.count > 0 && sg.tile_first >= 0 && sg.tile_first + sg.count <= jobs[sg.job].ntiles, "%s: segment out of range", what);
    CHECK(sg.gtile0 == gid, "%s: gtile0 %d after %d tiles", what, sg.gtile0, gid);
    for (int t = sg.tile_first; t < sg.tile_first + sg.count; ++t) ++seen[sg.job][t];
    gid += sg.count;
  }
  CHECK(gid == T, "%s: %d tile ids for %d tiles", what, gid, T);
  for (int i = 0; i < n; ++i)
    for (int t = 0; t < jobs[i].ntiles; ++t) CHECK(seen[i][t] == 1, "%s: tile %d of job %d listed %d times", what, t, i, seen[i][t]);
  // reductions fall along the tile ids (whole-tile rounds homogeneous, the shortest products in the remainder)
  for (size_t k = 1; k < segs.size(); ++k) CHECK(jobs[segs[k].job].nk <= jobs[segs[k - 1].job].nk, "%s: reduction lengths not falling", what);
  for (int G : {256, 240, 192}) {
    const int F = T / G, Rm = T - F * G;
    const int min_nk = tn_group_min_nk(jobs, segs, F * G);
    const int sp = tn_group_splits(Rm, G, min_nk);
    CHECK(sp >= 1 && sp <= 16, "%s: G %d: %d splits", what, G, sp);
    CHECK((int64_t)(sp - 1) * Rm <= kTnMaxFollowers, "%s: G %d: %d splits of %d remainder tiles", what, G, sp, Rm);
    // the kernel deals a tile's nk / 4 units of four stages evenly over the splits: a split tile has pieces of at least 16 stages;
    // a tile that is not split (sp = 1) is one piece whatever its length
    if (sp > 1) CHECK(min_nk / 4 >= 4 * sp, "%s: G %d: %d splits of %d stages", what, G, sp, min_nk);
    else if (Rm > 0) {
      CHECK(min_nk / 4 >= 1, "%s: G %d: %d stages", what, G, min_nk);
      g_unsplit_short += min_nk / 4 < 4;
    }
  }
  ++g_lists;
}

static hct_gemm_args product(int kind, int M, int N, int K, int c_dtype, bool colsum, int extra) {
  hct_gemm_args a;
  memset(&a, 0, sizeof(a));
  a.M = M; a.N = N; a.K = K;
  const int dt = kind == 2 ? HCT_F32 : HCT_BF16;
  a.A = kPtr; a.a_dtype = dt; a.B = kPtr; a.b_dtype = dt;
  if (kind == 1) { a.lda = M; a.transA = 1; a.ldb = N; a.transB = 0; }
  else { a.lda = K; a.transA = 0; a.ldb = K; a.transB = 1; }
  a.C = kPtr; a.c_dtype = c_dtype; a.ldc = N;
  a.alpha = 1.0f;
  if (colsum) a.colsum_out = (float*)kPtr;
  if (extra == 1) { a.residual = (const float*)kPtr; a.ldr = N; }
  if (extra == 2) { a.act = HCT_ACT_GELU; a.aux = kPtr; a.aux_dtype = HCT_BF16; a.ldaux = N; }
  if (extra == 3) { a.act = HCT_ACT_DGELU; a.aux = kPtr; a.aux_dtype = HCT_BF16; a.ldaux = N; }
  if (extra == 4) { a.C2 = kPtr; a.c2_dtype = HCT_BF16; a.ldc2 = N; }
  return a;
}

static long check_plans() {
  const int Ms[] = {16, 192, 200, 1000, 4096, 14080, 14144, 55552, 55616, 100000}, Ns[] = {16, 48, 768, 1000, 2304, 3072};
  const int Ks[] = {32, 64, 128, 448, 512, 768, 2304, 3072, 14080, 55552}, Gs[] = {256, 248, 240, 192, 64, 8};
  GemmTuning tunings[4];
  tunings[1].nt_variant = 128;
  tunings[2].sk_gain_pairs = 1;
  tunings[3].mt3 = false; tunings[3].sk_min_k = 1 << 30;
  long plans = 0;
  for (int kind = 0; kind < 3; ++kind) for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int cd : {HCT_F32, HCT_BF16})
    for (int colsum = 0; colsum < 2; ++colsum) for (int extra = 0; extra < 5; ++extra) for (int G : Gs) for (const GemmTuning& t : tunings) {
      const hct_gemm_args a = product(kind, M, N, K, cd, colsum, extra);
      const GemmPlan p = plan_gemm(&a, G, t, kUnlimited);
      const size_t ws = p.workspace_bytes;
      const bool tn = p.kernel == GEMM_TN128 || p.kernel == GEMM_TN256;
      CHECK(p.tiles >= 1 && p.grid >= 1 && (p.grid <= p.tiles || p.sk_tiles) && p.splits >= 1, "tiles %d grid %d splits %d", p.tiles, p.grid, p.splits);
      if (p.kernel == GEMM_NT256 || p.kernel == GEMM_TN256) CHECK(p.grid <= G, "grid %d on %d CUs", p.grid, G);
      if (tn) {
        CHECK(ws == p.slab_bytes && p.slab_bytes == (p.splits > 1 ? (size_t)p.splits * M * N * 4 : 0), "slab %zu", p.slab_bytes);
        CHECK(p.r_chunk > 0 && (int64_t)p.splits * p.r_chunk >= K && (int64_t)(p.splits - 1) * p.r_chunk < K, "%d splits of %d rows for K %d", p.splits, p.r_chunk, K);
      } else {
        CHECK(p.slab_bytes == 0 && ws >= p.colsum_bytes, "workspace %zu, column sums %zu", ws, p.colsum_bytes);
      }
      if (p.sk_tiles) {  // the region lies behind the column sums, inside the workspace, and the whole grid takes part
        CHECK(p.kernel == GEMM_NT256 && p.row_tiles_per_wave == 4 && p.grid == G && p.sk_tiles == p.tiles % G && p.sk_tiles < 256 && p.sk_wgs >= 1 &&
              p.sk_wgs <= G / 8, "stream-K %d tiles, %d workgroups per XCD", p.sk_tiles, p.sk_wgs);
        CHECK(p.stream_k_offset % 256 == 0 && p.stream_k_offset >= p.colsum_bytes && p.stream_k_offset + kSkBytes <= ws, "offset %zu of %zu", p.stream_k_offset, ws);
      } else {
        CHECK(p.stream_k_offset == kNoOffset && ws == (tn ? p.slab_bytes : p.colsum_bytes), "no stream-K, workspace %zu", ws);
      }
      if (p.row_tiles_per_wave == 3) CHECK(p.tiles == ceil_div(M, 192) * ceil_div(N, 256) && p.tiles <= G && p.grid == p.tiles, "192-row tiles: %d", p.tiles);
      // the request does not depend on what the caller has; the plan for exactly the request is the plan for plenty; a workspace
      // with no room for the region gets whole tiles, one with more room keeps the region at its end
      for (size_t avail : {(size_t)0, ws ? ws - 1 : 0, ws, ws + 1000, ws + kSkBytes + 12345}) {
        const GemmPlan q = plan_gemm(&a, G, t, avail);
        CHECK(q.workspace_bytes == ws && q.kernel == p.kernel && q.colsum_bytes == p.colsum_bytes && q.slab_bytes == p.slab_bytes, "request changed with the workspace");
        if (avail >= ws) {
          CHECK(q.sk_tiles == p.sk_tiles && q.sk_wgs == p.sk_wgs && q.grid == p.grid && q.tiles == p.tiles, "plan changed with a larger workspace");
          if (q.sk_tiles) CHECK(q.stream_k_offset == ws_layout(0, avail).stream_k_offset && q.stream_k_offset + kSkBytes <= avail && q.stream_k_offset >= p.colsum_bytes, "offset");
        } else {
          CHECK(q.sk_tiles == 0 && q.stream_k_offset == kNoOffset, "stream-K in a workspace of %zu < %zu", avail, ws);
        }
        ++plans;
      }
    }
  return plans;
}

int main() {
  // the five job lists of tests/test_kernels_gpu.py::test_gemm_tn_group
  check_group({{2000, 768, 3072}, {2000, 3072, 768}, {2016, 768, 768}, {2000, 2304, 768}}, "stream_k_only");
  {
    std::vector<Shape> s(5, Shape{300, 1536, 3072});
    s.insert(s.end(), 3, Shape{1000, 3072, 1536});
    check_group(s, "rounds_plus_remainder");
  }
  check_group({{130, 48, 64}, {33, 16, 16}, {4000, 272, 528}, {257, 768, 16}}, "mixed_small");
  check_group({{5000, 256, 256}}, "one_tile");
  check_group({{2000, 768, 3072}, {2000, 3072, 768}, {2016, 768, 768}, {2000, 2304, 768}}, "reserve16");
  // the MAE step's weight gradients (configs/mae/mae_HeadCT.yaml: ViT-B encoder, 12 blocks of 768 / 3072 on 256 x 55 = 14 080 token
  // rows; decoder, 8 blocks on 256 x 217 = 55 552; patch embedding, decoder embedding and prediction head), in backward order
  {
    std::vector<Shape> s;
    s.push_back({55552, 4096, 768});
    for (int b = 0; b < 8; ++b)
      for (Shape w : {Shape{55552, 768, 3072}, Shape{55552, 3072, 768}, Shape{55552, 768, 768}, Shape{55552, 2304, 768}}) s.push_back(w);
    s.push_back({14080, 768, 768});
    for (int b = 0; b < 12; ++b)
      for (Shape w : {Shape{14080, 768, 3072}, Shape{14080, 3072, 768}, Shape{14080, 768, 768}, Shape{14080, 2304, 768}}) s.push_back(w);
    s.push_back({13824, 768, 4096});
    check_group(s, "mae step");
  }
  std::mt19937 rng(20240613u);
  auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };
  for (int it = 0; it < 400; ++it) {
    std::vector<Shape> s(pick(1, 64));
    const bool few_lengths = it % 2;  // (classes of equal reduction length are what the window packing works on)
    const int lengths[3] = {pick(33, 60000), pick(33, 60000), pick(33, 60000)};
    for (Shape& w : s) w = Shape{few_lengths ? lengths[pick(0, 2)] : pick(33, 60000), 16 * pick(1, 256), 16 * pick(1, 256)};
    check_group(s, "random");
  }
  const long plans = check_plans();
  printf("ok %ld job lists (%ld unsplit remainders shorter than 16 stages), %ld plans\n", g_lists, g_unsplit_short, plans);
  return 0;
}
