// LoRA adapters of the ViT backbone's attention (reference: src/models/attentionblock.py:6-22, 45-47, 57-59; TRAIN.LORA).
//
// What the reference computes.  lora_q(x) = x . (Bq . Aq)^T is a [B, N, D] tensor that is added to q [B, H, N, dh] after a RAW
// reshape to [B, H, N, dh] -- no permute.  With U = (x . A^T) . B^T of shape [N, D] per volume and D = H dh, the dh-wide block
//     r = n' H + h'   (= U[n', h' dh : (h'+1) dh])   goes to   q[head = r / N, token = r % N, :]
// and the same for v.  This is therefore NOT a low-rank update of the qkv weight, and it cannot be folded into the qkv product:
// the adapters get a path of their own, which is this file.
//
//   forward   T = x1 . [Aq; Av]^T  [M, 2r]  (hct_gemm; kept for the backward), then  U = T . B^T  is added IN PLACE into the q and v
//             slots of the [B, N, 3, H, dh] qkv buffer at the permuted (token, head) position: stored value + fp32 accumulator,
//             rounded once to the compute dtype (lora_rmw kernels, PERM = true).
//   backward  dU = the q / v slots of dqkv read back through the inverse permutation (lora_gather_kernel), dB = dU^T . T,
//             dT = dU . B, dA = dT^T . x1 (hct_gemm / the grouped weight-gradient launch), dx1 += dT . A (lora_rmw, PERM = false).
//
// lora_rmw_mfma_kernel (bf16, D % 64 == 0, r in {32, 64, 128}): every product here has a short reduction (K = r, or 2r for dx1), so
// the kernels are bound by their passes over the M x D data.  A wave owns a 64-column tile of the output and keeps the whole
// [64, K] tile of the small matrix in registers (K/2 VGPRs) while it streams 16-row strips of the tall operand straight from
// global memory into MFMA fragments (lane l reads 16 contiguous bytes of row l & 15: the four k-steps of a strip cover 256
// contiguous bytes of every row) -- nothing is shared between waves, so there is no LDS stage and no barrier.  The operands are
// swapped in the MFMA (the small matrix is the "A" operand) so that a lane's four accumulator registers are four CONSECUTIVE
// columns of one output row, and the columns are dealt to the subtiles so that two of them give a lane EIGHT consecutive columns:
// the read-modify-write is a 16-byte access per lane, a wave's two accesses complete the 128-byte line of a dh = 64 block.  The
// loads of the next strip are issued before the products and stores of the current one.  A destination element is written by exactly one lane of one wave: no atomics, the result
// does not depend on the launch geometry.
// Everything else (fp32, other shapes, other ranks) takes lora_rmw_generic_kernel: one thread per output element, fixed
// summation order.
#include "common.h"

using namespace hct;

namespace {

struct RmwArgs {
  const void* A[2];   // tall operands [M, K], row stride lda
  const void* Bm[2];  // small operands: element (n, k) of pair p at Bm[p][n * ldb_n + k * ldb_k]
  int np;             // pairs (PERM: pair z of the grid is scattered to slot 2z; otherwise the pairs are summed)
  int lda, ldb_n, ldb_k;
  int M, D, K;
  void* C;            // PERM: the qkv buffer [B, N, 3, H, dh]; otherwise [M, D] with row stride ldc
  int ldc;
  int Ntok, H, dh;
};

// element offset of output element (m, n) of pair / slot index z
template <bool PERM>
__device__ __forceinline__ size_t rmw_dest(const RmwArgs& a, int m, int n, int z) {
  if (!PERM) return (size_t)m * a.ldc + n;
  const int b = m / a.Ntok, nt = m - b * a.Ntok;
  const int hh = n / a.dh, e = n - hh * a.dh;
  const int r = nt * a.H + hh;
  const int head = r / a.Ntok, tok = r - head * a.Ntok;
  return ((size_t)(b * a.Ntok + tok) * 3 + 2 * z) * a.D + (size_t)head * a.dh + e;
}

template <typename T, bool PERM>
__global__ void __launch_bounds__(256) lora_rmw_generic_kernel(RmwArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)a.M * a.D) return;
  const int m = (int)(idx / a.D), n = (int)(idx - (int64_t)m * a.D);
  const int z = PERM ? blockIdx.z : 0;
  const int p0 = PERM ? z : 0, p1 = PERM ? z + 1 : a.np;
  float acc = 0.f;
  for (int p = p0; p < p1; ++p) {
    const T* A = (const T*)a.A[p] + (size_t)m * a.lda;
    const T* Bm = (const T*)a.Bm[p] + (size_t)n * a.ldb_n;
    for (int k = 0; k < a.K; ++k) acc = fmaf(to_f32(A[k]), to_f32(Bm[(size_t)k * a.ldb_k]), acc);
  }
  T* c = (T*)a.C + rmw_dest<PERM>(a, m, n, z);
  *c = from_f32<T>(to_f32(*c) + acc);
}

constexpr int kRowsPerWave = 256;  // 16 strips of 16 rows per wave: the small-matrix tile is loaded once per 16 strips

// KS: k-steps of 32 per pair (K = 32 KS); NP: pairs held in registers.  ldb_k == 1 (the small matrix is [D, K] row-major).
// Column order inside the wave's 64-column tile: MFMA row i of subtile j stands for column 32 (j >> 1) + 8 (i >> 2) + 4 (j & 1) + (i & 3),
// so the accumulators of subtiles 2g and 2g + 1 of a lane are EIGHT consecutive columns (one 16-byte read-modify-write).
template <int KS, int NP, bool PERM>
__global__ void __launch_bounds__(256) lora_rmw_mfma_kernel(RmwArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int n0 = blockIdx.x * 64;
  const int z = PERM ? blockIdx.z : 0;
  const int row_begin = (blockIdx.y * 4 + wave) * kRowsPerWave;
  if (row_begin >= a.M) return;
  const int row_end = min(row_begin + kRowsPerWave, a.M);
  bf16x8 bfr[NP][4][KS];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const bf16* Bm = (const bf16*)a.Bm[PERM ? z : p];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + 32 * (j >> 1) + 8 * (l15 >> 2) + 4 * (j & 1) + (l15 & 3);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) bfr[p][j][ks] = *reinterpret_cast<const bf16x8*>(Bm + (size_t)n * a.ldb_n + ks * 32 + lq * 8);
    }
  }
  bf16* C = (bf16*)a.C;
  // operands of one strip: the tall operands' fragments and the stored values the products are added to
  struct Strip {
    bf16x8 af[NP][KS];
    bf16x8 old[2];
    size_t off[2];
  };
  auto load_strip = [&](int row0, Strip& st) {
    const int m = row0 + l15;
    const int mc = m < a.M ? m : a.M - 1;  // (rows past M: a valid row is loaded, nothing is stored)
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const bf16* A = (const bf16*)a.A[PERM ? z : p] + (size_t)mc * a.lda + lq * 8;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) st.af[p][ks] = *reinterpret_cast<const bf16x8*>(A + ks * 32);
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      st.off[g] = rmw_dest<PERM>(a, mc, n0 + 32 * g + 8 * lq, z);
      st.old[g] = *reinterpret_cast<const bf16x8*>(C + st.off[g]);
    }
  };
  // the next strip's loads are issued before this strip's products and stores (a wave's strips touch disjoint rows)
  Strip cur, nxt;
  load_strip(row_begin, cur);
  for (int row0 = row_begin; row0 < row_end; row0 += 16) {
    const bool more = row0 + 16 < row_end;
    if (more) load_strip(row0 + 16, nxt);
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[p][j][ks], cur.af[p][ks], acc[j], 0, 0, 0);
    }
    if (row0 + l15 < a.M) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = (bf16)((float)cur.old[g][e] + acc[2 * g][e]);
          o[4 + e] = (bf16)((float)cur.old[g][4 + e] + acc[2 * g + 1][e]);
        }
        *reinterpret_cast<bf16x8*>(C + cur.off[g]) = o;
      }
    }
    if (more) cur = nxt;
  }
}

// dU[m, z D + n] = dqkv at the position the forward added U[m, n] of slot 2z to; four elements per thread
template <typename T>
__global__ void __launch_bounds__(256) lora_gather_kernel(const T* __restrict__ dqkv, T* __restrict__ dU, RmwArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int q4 = a.D / 4;
  if (idx >= (int64_t)a.M * q4) return;
  const int m = (int)(idx / q4), n = (int)(idx - (int64_t)m * q4) * 4;
  const int z = blockIdx.z;
  const f32x4 v = Vec4<T>::load(dqkv + rmw_dest<true>(a, m, n, z));
  Vec4<T>::store(dU + (size_t)m * 2 * a.D + (size_t)z * a.D + n, v);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool PERM>
int rmw_launch(const RmwArgs& a, int dt, hipStream_t s) {
  const int nz = PERM ? a.np : 1;
  bool mfma = dt == HCT_BF16 && a.D % 64 == 0 && a.ldb_k == 1 && a.ldb_n % 8 == 0 && a.lda % 8 == 0 && (a.K == 32 || a.K == 64 || a.K == 128) &&
              aligned16(a.C) && (PERM ? a.dh % 8 == 0 : a.ldc % 8 == 0) && (PERM || a.np == 2);
  for (int p = 0; p < a.np; ++p) mfma = mfma && aligned16(a.A[p]) && aligned16(a.Bm[p]);
  if (mfma) {
    const dim3 grid(a.D / 64, (a.M + 4 * kRowsPerWave - 1) / (4 * kRowsPerWave), nz);
#define HCT_LORA_MFMA(KS_)                                                                                             \
  hipLaunchKernelGGL((lora_rmw_mfma_kernel<KS_, PERM ? 1 : 2, PERM>), grid, dim3(256), 0, s, a)
    if (a.K == 128) HCT_LORA_MFMA(4);
    else if (a.K == 64) HCT_LORA_MFMA(2);
    else HCT_LORA_MFMA(1);
#undef HCT_LORA_MFMA
  } else {
    const int64_t n = (int64_t)a.M * a.D;
    const dim3 grid((unsigned)((n + 255) / 256), 1, nz);
    HCT_DISPATCH_DTYPE(dt, T, hipLaunchKernelGGL((lora_rmw_generic_kernel<T, PERM>), grid, dim3(256), 0, s, a));
  }
  return check_hip(hipGetLastError(), PERM ? "lora_scatter" : "lora_dx_accum");
}

int check_shape(const char* what, int B, int N, int H, int dh, int r, int dtype) {
  HCT_REQUIRE(B > 0 && N > 0 && H > 0 && dh > 0 && dh % 4 == 0, "%s: bad shape (B %d, N %d, H %d, dh %d; dh must be a multiple of 4)", what, B, N, H, dh);
  HCT_REQUIRE(r > 0 && r % 32 == 0, "%s: the LoRA rank must be a positive multiple of 32 (%d)", what, r);
  HCT_REQUIRE(dtype == HCT_F32 || dtype == HCT_BF16, "%s: dtype must be HCT_F32 or HCT_BF16", what);
  HCT_REQUIRE((int64_t)B * N * 3 * H * dh < (1ll << 40) && (int64_t)B * N < (1ll << 31), "%s: problem too large", what);
  return 0;
}

}  // namespace

namespace hct {

int lora_scatter(const void* T, int ldt, const void* Bq, const void* Bv, int B, int N, int H, int dh, int r, int dt, void* qkv, hipStream_t s) {
  RmwArgs a;
  memset(&a, 0, sizeof(a));
  const size_t es = dtype_size(dt);
  a.A[0] = T; a.A[1] = (const unsigned char*)T + (size_t)r * es;
  a.Bm[0] = Bq; a.Bm[1] = Bv;
  a.np = 2; a.lda = ldt; a.ldb_n = r; a.ldb_k = 1;
  a.M = B * N; a.D = H * dh; a.K = r;
  a.C = qkv; a.ldc = 3 * H * dh; a.Ntok = N; a.H = H; a.dh = dh;
  return rmw_launch<true>(a, dt, s);
}

int lora_gather(const void* dqkv, int B, int N, int H, int dh, int dt, void* dU, hipStream_t s) {
  RmwArgs a;
  memset(&a, 0, sizeof(a));
  a.M = B * N; a.D = H * dh; a.Ntok = N; a.H = H; a.dh = dh;
  const int64_t n = (int64_t)a.M * (a.D / 4);
  const dim3 grid((unsigned)((n + 255) / 256), 1, 2);
  HCT_DISPATCH_DTYPE(dt, T, hipLaunchKernelGGL(lora_gather_kernel<T>, grid, dim3(256), 0, s, (const T*)dqkv, (T*)dU, a));
  return check_hip(hipGetLastError(), "lora_gather");
}

// dx1[M, D] += dT[:, 0:r] . Aq + dT[:, r:2r] . Av.   transposed: Aq / Av point at the [D, r] transposed copies.
int lora_dx_accum(const void* dT, int ldt, const void* Aq, const void* Av, bool transposed, int M, int D, int r, int dt, void* dx1, hipStream_t s) {
  RmwArgs a;
  memset(&a, 0, sizeof(a));
  const size_t es = dtype_size(dt);
  a.A[0] = dT; a.A[1] = (const unsigned char*)dT + (size_t)r * es;
  a.Bm[0] = Aq; a.Bm[1] = Av;
  a.np = 2; a.lda = ldt;
  a.ldb_n = transposed ? r : 1; a.ldb_k = transposed ? 1 : D;
  a.M = M; a.D = D; a.K = r;
  a.C = dx1; a.ldc = D;
  return rmw_launch<false>(a, dt, s);
}

}  // namespace hct

namespace {

hct_gemm_args gemm_base(int dt) {
  hct_gemm_args g;
  memset(&g, 0, sizeof(g));
  g.alpha = 1.0f;
  g.a_dtype = g.b_dtype = dt;
  return g;
}

// T[:, c0 : c0 + r] = x1 . A^T
hct_gemm_args t_product(const void* x1, const void* A, int M, int D, int r, int dt, void* T, int c0) {
  hct_gemm_args g = gemm_base(dt);
  g.M = M; g.N = r; g.K = D;
  g.A = x1; g.lda = D; g.transA = 0;
  g.B = A; g.ldb = D; g.transB = 1;
  g.C = (unsigned char*)T + (size_t)c0 * dtype_size(dt); g.c_dtype = dt; g.ldc = 2 * r;
  return g;
}

// dT[:, c0 : c0 + r] = dU[:, u0 : u0 + D] . Bm      (Bt: the [r, D] transposed copy, or null)
hct_gemm_args dt_product(const void* dU, int u0, const void* Bm, const void* Bt, int M, int D, int r, int dt, void* dT, int c0) {
  hct_gemm_args g = gemm_base(dt);
  const size_t es = dtype_size(dt);
  g.M = M; g.N = r; g.K = D;
  g.A = (const unsigned char*)dU + (size_t)u0 * es; g.lda = 2 * D; g.transA = 0;
  if (Bt) { g.B = Bt; g.ldb = D; g.transB = 1; }
  else { g.B = Bm; g.ldb = r; g.transB = 0; }
  g.C = (unsigned char*)dT + (size_t)c0 * es; g.c_dtype = dt; g.ldc = 2 * r;
  return g;
}

// dW[rows, cols] = X[:, x0 : x0 + rows]^T . Y[:, y0 : y0 + cols]   (fp32 gradient, reduction over the M rows)
hct_gemm_args tn_product(const void* X, int x0, int ldx, int rows, const void* Y, int y0, int ldy, int cols, int M, int dt, float* dW) {
  hct_gemm_args g = gemm_base(dt);
  const size_t es = dtype_size(dt);
  g.M = rows; g.N = cols; g.K = M;
  g.A = (const unsigned char*)X + (size_t)x0 * es; g.lda = ldx; g.transA = 1;
  g.B = (const unsigned char*)Y + (size_t)y0 * es; g.ldb = ldy; g.transB = 0;
  g.C = dW; g.c_dtype = HCT_F32; g.ldc = cols;
  return g;
}

size_t bwd_gemm_ws(int M, int D, int r, int dt) {
  // alignment probes only: the workspace of a product depends on its shape and strides
  const void* probe = (const void*)256;
  hct_gemm_args g1 = tn_product(probe, 0, 2 * D, D, probe, 0, 2 * r, r, M, dt, (float*)256);
  hct_gemm_args g2 = tn_product(probe, 0, 2 * r, r, probe, 0, D, D, M, dt, (float*)256);
  size_t a = hct_gemm_workspace_bytes(&g1), b = hct_gemm_workspace_bytes(&g2);
  return align_up(a > b ? a : b, 256);
}

}  // namespace

extern "C" {

int hct_lora_qv_fwd(const void* x1, const void* Aq, const void* Av, const void* Bq, const void* Bv, int B, int N, int H, int dh, int r, int dtype,
                    void* T, void* qkv, void* stream) {
  if (int rc = check_shape("hct_lora_qv_fwd", B, N, H, dh, r, dtype)) return rc;
  HCT_REQUIRE(x1 && Aq && Av && Bq && Bv && T && qkv, "hct_lora_qv_fwd: null argument");
  const int M = B * N, D = H * dh;
  hct_gemm_args g = t_product(x1, Aq, M, D, r, dtype, T, 0);
  if (int rc = hct_gemm(&g, nullptr, 0, stream)) return rc;
  g = t_product(x1, Av, M, D, r, dtype, T, r);
  if (int rc = hct_gemm(&g, nullptr, 0, stream)) return rc;
  return lora_scatter(T, 2 * r, Bq, Bv, B, N, H, dh, r, dtype, qkv, (hipStream_t)stream);
}

size_t hct_lora_qv_bwd_workspace_bytes(int M, int D, int r, int dtype) {
  if (M <= 0 || D <= 0 || r <= 0) return 0;
  const size_t es = dtype_size(dtype);
  return align_up((size_t)M * 2 * D * es, 256) + align_up((size_t)M * 2 * r * es, 256) + bwd_gemm_ws(M, D, r, dtype);
}

int hct_lora_qv_bwd(const void* dqkv, const void* x1, const void* T, const void* Aq, const void* Av, const void* Bq, const void* Bv,
                    const void* AqT, const void* AvT, const void* BqT, const void* BvT, int B, int N, int H, int dh, int r, int dtype, float* dAq,
                    float* dAv, float* dBq, float* dBv, void* dx1, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_shape("hct_lora_qv_bwd", B, N, H, dh, r, dtype)) return rc;
  HCT_REQUIRE(dqkv && x1 && T && Aq && Av && Bq && Bv && dAq && dAv && dBq && dBv && dx1 && workspace, "hct_lora_qv_bwd: null argument");
  HCT_REQUIRE((AqT != nullptr) == (AvT != nullptr) && (BqT != nullptr) == (BvT != nullptr), "hct_lora_qv_bwd: transposed copies come in pairs");
  const int M = B * N, D = H * dh;
  if (workspace_bytes < hct_lora_qv_bwd_workspace_bytes(M, D, r, dtype)) {
    set_error("hct_lora_qv_bwd: workspace too small (%zu < %zu)", workspace_bytes, hct_lora_qv_bwd_workspace_bytes(M, D, r, dtype));
    return HCT_E_WORKSPACE;
  }
  const size_t es = dtype_size(dtype);
  hipStream_t s = (hipStream_t)stream;
  unsigned char* dU = (unsigned char*)workspace;
  unsigned char* dT = dU + align_up((size_t)M * 2 * D * es, 256);
  unsigned char* gws = dT + align_up((size_t)M * 2 * r * es, 256);
  const size_t gws_bytes = bwd_gemm_ws(M, D, r, dtype);
  if (int rc = lora_gather(dqkv, B, N, H, dh, dtype, dU, s)) return rc;
  for (int z = 0; z < 2; ++z) {
    hct_gemm_args g = tn_product(dU, z * D, 2 * D, D, T, z * r, 2 * r, r, M, dtype, z ? dBv : dBq);
    if (int rc = hct_gemm(&g, gws, gws_bytes, stream)) return rc;
    g = dt_product(dU, z * D, z ? Bv : Bq, z ? BvT : BqT, M, D, r, dtype, dT, z * r);
    if (int rc = hct_gemm(&g, nullptr, 0, stream)) return rc;
  }
  for (int z = 0; z < 2; ++z) {
    hct_gemm_args g = tn_product(dT, z * r, 2 * r, r, x1, 0, D, D, M, dtype, z ? dAv : dAq);
    if (int rc = hct_gemm(&g, gws, gws_bytes, stream)) return rc;
  }
  const bool tr = AqT != nullptr && dtype == HCT_BF16;
  return lora_dx_accum(dT, 2 * r, tr ? AqT : Aq, tr ? AvT : Av, tr, M, D, r, dtype, dx1, s);
}

}  // extern "C"
