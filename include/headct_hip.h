/*
 * headct_hip.h -- C ABI of libheadct_hip.so: the MI355X (gfx950) MAE pre-training hot path.
 *
 * The reference (nirvanesque/headCT_foundation) has no FFI seam: the hot path sits behind the
 * Python nn.Module contract of MaskedAutoencoderViT and the engine_pretrain_mae functions
 * (SURVEY.md 8b).  This header is the boundary a maintainer would bind instead of the PyTorch
 * operators that path dispatches today; each entry point cites the reference lines it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns all memory,
 *     the library never allocates or frees device memory;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); calls are asynchronous;
 *   - return value: 0 on success, a positive hipError_t, or a negative HCT_E_* code;
 *     hct_last_error_string() gives text for the calling thread's last failure;
 *   - dtype codes: HCT_F32 = 0 (fp32 storage), HCT_BF16 = 1 (bfloat16 storage, fp32 accumulation);
 *   - matrices are row-major; "ld" = row stride in elements.
 */
#ifndef HEADCT_HIP_H
#define HEADCT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HCT_F32 0
#define HCT_BF16 1
#define HCT_F16 2 /* IEEE half: input volumes of the persistent cache only (hct_augment_volume) */

#define HCT_E_BADARG (-1)
#define HCT_E_UNSUPPORTED (-2)
#define HCT_E_WORKSPACE (-3)
#define HCT_E_STATE (-4)

#define HCT_ACT_NONE 0
#define HCT_ACT_GELU 1  /* out = gelu_erf(acc + bias); aux (if given) receives the pre-activation */
#define HCT_ACT_DGELU 2 /* out = acc * gelu_erf'(aux)   (aux = saved pre-activation)             */
#define HCT_ACT_TANH 3  /* hct_head_linear only: out = tanh(acc + bias)                           */
#define HCT_ACT_GELU_D 4 /* hct_gemm: out = gelu_erf(acc + bias); aux receives gelu_erf'(acc + bias) -- what the backward     */
#define HCT_ACT_MULAUX 5 /* hct_gemm: out = acc * aux -- needs (the derivative is evaluated once, on the unrounded value)   */

const char* hct_last_error_string(void);
int hct_version(void);
/* 1 when the tuned gfx950 MFMA kernels are compiled in (always, in this build). */
int hct_has_mfma_kernels(void);

/* ------------------------------------------------------------------------------------------
 * GEMM with fused epilogue:  C = act(alpha * op(A) . op(B) + bias) (+ residual)
 * Replaces nn.Linear / Conv3d-as-GEMM forward and the autograd dgrad / wgrad products
 * (attentionblock.py:41-42,54,64; MONAI MLPBlock linear1/linear2; mae.py:118-119;
 *  patch_embedding.py:102-105,149).
 *   transA = 0: A stored [M,K];  transA = 1: A stored [K,M]  (op(A) = A^T)
 *   transB = 1: B stored [N,K] (the nn.Linear weight layout, "NT"); transB = 0: B stored [K,N]
 * Dispatch: bf16 x bf16, transA=0, transB=1, K%64==0, N%16==0 -> tuned MFMA "NT" kernel;
 *           bf16 x bf16, transA=1, transB=0, M%16==0, N%16==0   -> tuned MFMA "TN" kernel (split-K
 *           over the reduction, partial slabs in `workspace`, deterministic reduction);
 *           anything else (all fp32 work) -> generic strided kernel (fp32 FMA accumulation).
 * ------------------------------------------------------------------------------------------ */
typedef struct hct_gemm_args {
  int M, N, K;
  const void* A; int a_dtype; int64_t lda; int transA;
  const void* B; int b_dtype; int64_t ldb; int transB;
  void* C; int c_dtype; int64_t ldc;
  const float* bias;     /* [N] fp32 or NULL */
  const float* residual; /* [M,N] fp32 (row stride ldr) or NULL; added after the activation */
  int64_t ldr;
  int act;               /* HCT_ACT_* */
  void* aux; int aux_dtype; int64_t ldaux;
  void* C2; int c2_dtype; int64_t ldc2; /* optional second copy of the output (e.g. bf16 shadow) */
  float alpha;
  int force_generic;     /* testing: always take the generic kernel */
  float* colsum_out;     /* optional [N] fp32: column sums of the OUTPUT C (the bias gradient of the Linear that produced the
                            operand of this dgrad); fused into the epilogue where the kernel supports it (sums of the unrounded
                            values), otherwise a separate pass over C as stored.  Needs N % 4 == 0, ldc % 4 == 0, C aligned to
                            four elements and a workspace; not on the "TN" path.  Refused (HCT_E_BADARG / HCT_E_WORKSPACE)
                            before anything is launched otherwise: no output is touched. */
  int workspace_armed;   /* NT path: 1 = the head of the stream-K region (hct_gemm_nt_flags_offset) was zero when first used and
                            has only been touched by hct_gemm since: skips the per-call reset.  0 = reset it. */
} hct_gemm_args;

size_t hct_gemm_workspace_bytes(const hct_gemm_args* a);
/* NT path (forward Linears / dgrads), persistent 256x256 kernel: when the tile count leaves a partly filled last round, the
 * remainder tiles are shared out by K range over all CUs ("stream-K"; whole tiles for the rest), partial accumulators passing
 * through the LAST 64 MiB + 4 KiB of `workspace` in a fixed summation order (bit-reproducible).  Optional: with a smaller (or
 * no) workspace the launch uses whole tiles only.  hct_gemm_workspace_bytes includes the region only for shapes whose
 * remainder round would be shared out on the present CU count.  An owner that waits in vain for a partial (a grid that is
 * not wholly resident) sets the error word AND fills its tile with NaN.  hct_gemm_nt_flags_offset = byte offset of that region's head inside a
 * workspace of the given size ((size_t)-1: too small): 256 32-bit arrival flags, and at byte 2048 an error word that a launch
 * sets to 0xDEAD if a partial never arrived (cannot happen while the grid is resident; it is flagged rather than waited for).
 * The head is reset before every such launch unless `workspace_armed` says that it started zeroed and only hct_gemm has
 * written it since.  The sharing is used where it saves at least 20 K-stage pairs per CU (tuned on the MAE step). */
size_t hct_gemm_nt_flags_offset(size_t workspace_bytes);
size_t hct_gemm_nt_stream_k_bytes(void); /* size of that region: what a caller that keeps ONE workspace for many shapes appends to it */
/* Leave `n` CUs out of the persistent GEMM grids (default 0) so that communication kernels (RCCL all-reduce overlapped
 * with the backward) have somewhere to run; set by the data-parallel wrapper when world_size > 1. */
void hct_set_cu_reserve(int n);
int hct_gemm(const hct_gemm_args* a, void* workspace, size_t workspace_bytes, void* stream);
/* What hct_gemm would launch for `a` on `num_cus` CUs (<= 0: the count the library uses) with `workspace_bytes` of workspace
 * ((size_t)-1: as much as it asks for).  Host arithmetic only (no device call): the plan hct_gemm itself launches from. */
#define HCT_GEMM_GENERIC 0 /* strided fp32-FMA kernel, 64x64 tiles */
#define HCT_GEMM_NT128 1   /* 128x128 tiles, one per workgroup */
#define HCT_GEMM_NT256 2   /* persistent 256x256 (or 192x256) tiles */
#define HCT_GEMM_TN128 3   /* wgrad, 128x128 tiles, grid.y = splits */
#define HCT_GEMM_TN256 4   /* wgrad, persistent 256x256 tiles x splits */
typedef struct hct_gemm_plan_info {
  int kernel;             /* HCT_GEMM_* */
  int epilogue_mode;      /* NT256: epilogue instance (0 generic, 1 plain bf16, 2 +residual fp32, 3 GELU, 4 x GELU') */
  int fuse_colsum;        /* NT256: colsum_out comes from the epilogue (else a separate pass over C) */
  int row_tiles_per_wave; /* NT256: 4 = 256-row tiles, 3 = 192-row tiles */
  int tiles, grid;        /* output tiles (TN256: x splits) and workgroups (TN128: grid.x) */
  int sk_tiles, sk_wgs;   /* NT256 stream-K: remainder tiles shared out by K range, workgroups per XCD that take a range (0: whole tiles) */
  int splits, r_chunk;    /* TN: split-K pieces and reduction rows per piece */
  size_t colsum_bytes;    /* column-sum partials at the head of the workspace */
  size_t stream_k_offset; /* of the stream-K region inside the workspace, (size_t)-1: none */
  size_t slab_bytes;      /* TN: split-K partial slabs */
  size_t workspace_bytes; /* = hct_gemm_workspace_bytes(a) */
  int walk_width;         /* NT256: column tiles per band of the tile walk (= all of N's: n fastest over the whole row, no bands) */
} hct_gemm_plan_info;
int hct_gemm_describe(const hct_gemm_args* a, int num_cus, size_t workspace_bytes, hct_gemm_plan_info* out);
/* The stream-K work items of every workgroup of an NT256 launch (grid workgroups, `pairs` = K / 64 stage pairs per tile), computed
 * by the function the kernel calls: first[wg] / owner[wg] = packed item the workgroup computes first / an owner piece it computes
 * second, 0 = none; tile id [0,8) | first pair [8,18) | pairs [18,28) | followers to collect [28,31) | bit 31: owns the tile. */
int hct_gemm_stream_k_items(int grid, int sk_tiles, int sk_wgs, int pairs, uint32_t* first, uint32_t* owner);
/* The whole-tile walk of an NT256 launch, computed by the functions the kernel calls: ids[vb] for every virtual block id
 * vb in [0, tiles - sk_tiles) (workgroup b takes vb = b, b + grid, ...; XCD = vb & 7) = tile id (row tile * n_col_tiles + column
 * tile) in [sk_tiles, tiles); `walk_width` as in the plan. */
int hct_gemm_nt_walk(int tiles, int n_col_tiles, int sk_tiles, int walk_width, int* ids);
/* Grouped weight gradients: n "TN" products dW_i[M_i,N_i] = alpha_i * A_i[K_i,M_i]^T . B_i[K_i,N_i] (bf16 operands, fp32 C, no
 * epilogue extras) in ONE persistent launch, each 256x256 output tile reducing over ALL K_i rows (no split partials, no fold
 * launch); the partly filled last round of tiles is shared out by reduction range with a fixed summation order
 * (bit-reproducible).  The weight gradients of a training step do not feed its backward chain, so the model driver collects
 * those of several blocks and runs them here (the reference computes each inside autograd's backward of its Linear,
 * attentionblock.py:41-42, MLPBlock).  `prepare` writes the job table into the workspace and zeroes its flags (once per set of
 * pointers / shapes, stream-ordered); `run` launches on the prepared table (same jobs array).  workspace: 256-byte aligned,
 * hct_gemm_tn_group_workspace_bytes(n), used by nothing else between prepare and the last run.                              */
size_t hct_gemm_tn_group_workspace_bytes(int n_jobs);
int hct_gemm_tn_group_prepare(const hct_gemm_args* jobs, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);
int hct_gemm_tn_group_run(const hct_gemm_args* jobs, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Random masking from supplied noise (mae.py:204-216).  Stable ranking: ties -> lower index first.
 *   noise [B,L] fp32  ->  ids_restore [B,L] i32, ids_shuffle [B,L] i32 (first K = ids_keep),
 *   mask [B,L] fp32 (0 keep, 1 masked).
 * ------------------------------------------------------------------------------------------ */
int hct_mask_rank(const float* noise, int B, int L, int K, int32_t* ids_restore, int32_t* ids_shuffle,
                  float* mask, void* stream);

/* ------------------------------------------------------------------------------------------
 * Patch gather (im2col of the stride==kernel Conv3d, kept tokens only; patch_embedding.py:149-152
 * + mae.py:212).   x [B,C,S,S,S] fp32 -> rows [B*K, C*P^3] in Conv3d weight order (c,ph,pw,pd).
 * ------------------------------------------------------------------------------------------ */
int hct_patch_gather(const void* x, int x_dtype /* HCT_F32 | HCT_F16 */, const int32_t* ids_shuffle, int B, int C, int S, int P, int L, int K,
                     void* rows, int rows_dtype, void* stream);

/* Encoder input assembly: h0[b,0,:] = cls;  h0[b,1+j,:] = tok[b*K+j,:] + pos[ids_keep[b,j],:]
 * (patch_embedding.py:155-156, mae.py:212,233-234).  pos may be NULL (pos_embed == "none").   */
int hct_encoder_assemble_fwd(const void* tok, int tok_dtype, const float* cls, const float* pos,
                             const int32_t* ids_shuffle, int B, int L, int K, int D, float* h0, void* stream);
/* backward: dtok[b*K+j] = dh0[b,1+j]; dcls = sum_b dh0[b,0]; dpos[l] = sum_{b: l kept} dh0[b,1+rank]. */
int hct_encoder_assemble_bwd(const float* dh0, const int32_t* ids_restore, int B, int L, int K, int D,
                             void* dtok, int dtok_dtype, float* dcls, float* dpos, void* workspace,
                             size_t workspace_bytes, void* stream);
/* workspace for the *_assemble_bwd reductions */
size_t hct_assemble_bwd_workspace_bytes(int D);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dim.  eps is the caller's: 1e-5 in the MAE (nn.LayerNorm default; attentionblock.py:92-93,
 * mae.py:116-117), 1e-6 on the ViT path (vit.py hands in its ln.eps).  x fp32 [rows,D] (the residual stream); y in y_dtype;
 * mean/rstd saved fp32.
 * ------------------------------------------------------------------------------------------ */
int hct_layernorm_fwd(const float* x, const float* gamma, const float* beta, int rows, int D, float eps,
                      void* y, int y_dtype, float* mean, float* rstd, void* stream);
/* dx_total = dres + LN'(dy)  written fp32 to dx (may alias dres) and, if dx_shadow != NULL, also
 * in shadow_dtype.  dgamma/dbeta [D] fp32 (overwritten); if dcolsum != NULL it receives
 * sum_rows(dx_total) [D] (the bias gradient of the Linear that produced this residual branch).
 * workspace: hct_layernorm_bwd_workspace_bytes(rows, D).                                       */
size_t hct_layernorm_bwd_workspace_bytes(int rows, int D);
int hct_layernorm_bwd(const void* dy, int dy_dtype, const float* x, const float* mean, const float* rstd,
                      const float* gamma, const float* dres, int rows, int D, float* dx, void* dx_shadow,
                      int shadow_dtype, float* dgamma, float* dbeta, float* dcolsum, void* workspace,
                      size_t workspace_bytes, void* stream);
/* The same with the residual gradient taken from a COMPACT matrix: row r adds dres[dres_rows[r]], nothing where
 * dres_rows[r] < 0 (dres_rows == NULL: as hct_layernorm_bwd).  dres must not alias dx then.  Used by the plan where the
 * tail of the MAE decoder runs on the masked patches' rows only (mae.py:298-299: the loss takes no other row).      */
int hct_layernorm_bwd_mapped(const void* dy, int dy_dtype, const float* x, const float* mean, const float* rstd,
                             const float* gamma, const float* dres, const int32_t* dres_rows, int rows, int D, float* dx,
                             void* dx_shadow, int shadow_dtype, float* dgamma, float* dbeta, float* dcolsum, void* workspace,
                             size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------------------------------
 * RMSNorm over the last dim (src/models/layers.py:11-54): y = x * rsqrt(mean_d(x^2) + eps) * gamma, statistics in fp32,
 * no mean subtraction and no bias (:40, :53-54); eps = 1e-6 wherever the reference builds one (class default :12;
 * vit.py:124).  x fp32 [rows,D]; y in y_dtype; rstd saved fp32 (the only statistic).
 * ------------------------------------------------------------------------------------------ */
int hct_rmsnorm_fwd(const float* x, const float* gamma, int rows, int D, float eps, void* y, int y_dtype, float* rstd,
                    void* stream);
/* dx_total = dres + RMSNorm'(dy), with xhat = x rstd, a = dy gamma:  RMSNorm'(dy) = rstd (a - xhat mean_d(a xhat)).
 * Everything else as hct_layernorm_bwd[_mapped]: dx fp32 (may alias dres in the plain call), optional shadow, dgamma [D]
 * overwritten, optional dcolsum = sum_rows(dx_total), dres_rows < 0 = no residual gradient for that row; D <= 1024.  */
size_t hct_rmsnorm_bwd_workspace_bytes(int rows, int D);
int hct_rmsnorm_bwd(const void* dy, int dy_dtype, const float* x, const float* rstd, const float* gamma, const float* dres,
                    int rows, int D, float* dx, void* dx_shadow, int shadow_dtype, float* dgamma, float* dcolsum,
                    void* workspace, size_t workspace_bytes, void* stream);
int hct_rmsnorm_bwd_mapped(const void* dy, int dy_dtype, const float* x, const float* rstd, const float* gamma,
                           const float* dres, const int32_t* dres_rows, int rows, int D, float* dx, void* dx_shadow,
                           int shadow_dtype, float* dgamma, float* dcolsum, void* workspace, size_t workspace_bytes,
                           void* stream);
/* Rows of the [B, L+1] decoder layout that hold masked patches (mae.py:207-214: ids_restore[b, l] >= K), per volume in
 * shuffle order: tail_rows [B*(L-K)] and its inverse tail_inv [B*(L+1)] (-1 for the class token and the kept patches). */
int hct_tail_rows(const int32_t* ids_restore, int B, int L, int K, int32_t* tail_rows, int32_t* tail_inv, void* stream);
/* dst row r = src row idx[r], zeros where idx[r] < 0; rows of row_bytes (multiple of 16) bytes, 16-byte aligned bases.  */
int hct_gather_rows(const void* src, const int32_t* idx, int n_rows, int row_bytes, void* dst, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-head self-attention, no mask, scale dh^-1/2 (attentionblock.py:54-62,
 * F.scaled_dot_product_attention).  qkv [B,N,3,H,dh] (the fused-QKV Linear output, as the
 * reference views it :54); o [B,N,H*dh] (head-merged, as :62); lse [B,H,N] fp32 saved for backward.
 * dtype = storage of qkv / o / do / dqkv.
 * ------------------------------------------------------------------------------------------ */
int hct_attention_fwd(const void* qkv, int B, int N, int H, int dh, int dtype, void* o, float* lse, void* stream);
int hct_attention_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, int B, int N, int H,
                      int dh, int dtype, void* dqkv, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dropout (training mode of attentionblock.py:61 / :65 / :97-98, patch_embedding.py:160, MONAI MLPBlock).  Keep masks are never
 * stored: they are a function of (seed, site, element), drawn again wherever they are needed.
 *   generator  Philox4x32-10, key = the 64-bit seed (low word, high word)
 *   streaming  element e of the row-major tensor the site acts on: counter (low32(e >> 2), high32(e >> 2), 0, site), word e & 3
 *   attention  score (b, h, q, k): counter (k >> 2, q, b * H + h, site), word k & 3
 *   keep rule  keep iff word >= T, T = floor(p * 2^32) of the fp32 value p; kept values are scaled by 1 / (1 - p) in fp32
 * 0 <= p < 1; p = 1 is refused by name (HCT_E_BADARG).  `site` is a small non-negative integer that tells the uses of one seed apart.
 *
 * hct_dropout_mask: the keep mask as bytes (1 keep, 0 drop), for tests and debugging -- kind 0: a streaming tensor of n elements;
 *   kind 1: the attention probabilities [BH, N, N] (BH = B * H).  The fused kernels agree with it bit for bit.
 * hct_dropout_apply: y = x o Z (+ residual, fp32, then y is fp32) and, if given, y2 = x2 o Z with the same mask, on `batches`
 *   segments of `seg` elements that start at element b * stride + off of the tensor the site acts on; x and x2 of x_dtype, y and y2
 *   of y_dtype (fp32 / bf16), y may be x and y2 may be x2.  off % 4 == 0, and with more than one segment stride % 4 == 0; base
 *   pointers 16-byte aligned.  The whole tensor is batches = 1, off = 0, seg = n.  The backward is the same call on the gradient.
 * hct_attention_dropout_fwd / _bwd: hct_attention_fwd / _bwd with O = (softmax(S) o Z) V; lse is that of the undropped probabilities.
 *
 * Stochastic depth (drop path; hct_mae_config.drop_path_rate): one decision per (sample, residual branch) from the same seed.
 *   rates      block j of `depth` blocks at rate r (the fp32 value) has q_j = r * j / (depth - 1), evaluated in double and cast to fp32;
 *              q_0 = 0 and a one-block model has q = [0].  Both residual branches of block j use q_j.  0 <= r < 1.
 *   decision   sample b (index along the batch axis) at a branch: counter (b >> 2, 0, 1, site), word b & 3, same key; kept iff
 *              word >= floor(q * 2^32); its multiplier s_b is 1 / (1 - q) in fp32 when kept, else 0.  `site` is the branch's streaming
 *              site: 1 + 4 j + 1 (attention branch, the proj_drop site), 1 + 4 j + 3 (MLP branch, the drop2 site).  The third counter
 *              word is 1 where the streaming element masks have 0, so the two families never share a counter at one site.
 *              At q = 0 the multiplier is exactly 1.0 and nothing is drawn.
 *   block      h_mid = h_in + (proj(o) o Z_proj) * s^attn_b,  h_out = h_mid + (linear2(g) o Z_drop2) * s^mlp_b
 *   arithmetic one combined fp32 multiplier per element, c = fl(z * s_b) with z in {0, 1 / (1 - p)}; y = fl(fl(x * c) + residual).
 * hct_drop_path_scales: out [n_sites, B] fp32 (device) <- the multipliers s_b of `n_sites` branches; `sites` and `rates` are HOST
 *   arrays of n_sites entries (they travel as kernel arguments: one launch per 128 rows).
 * hct_residual_drop_apply: y = x o Z(site, p) * scales[b] (+ residual, fp32, then y is fp32) on a tensor of B segments of `seg`
 *   elements, segment b being sample b; `scales` is one row of the table above (device, B floats).  x of x_dtype, y of y_dtype (fp32 /
 *   bf16), y may be x.  With B > 1 seg % 4 == 0 (a group of four elements never straddles two samples); base pointers 16-byte
 *   aligned.  At p = 0 no element mask is drawn: the multiplier is the table value alone.  The backward is the same call on the gradient.
 * ------------------------------------------------------------------------------------------ */
int hct_dropout_mask(uint64_t seed, int site, int kind, int64_t n, int BH, int N, float p, unsigned char* out, void* stream);
int hct_dropout_apply(const void* x, int x_dtype, void* y, int y_dtype, const float* residual, const void* x2, void* y2,
                      int64_t batches, int64_t stride, int64_t off, int64_t seg, uint64_t seed, int site, float p, void* stream);
int hct_attention_dropout_fwd(const void* qkv, int B, int N, int H, int dh, int dtype, float p, uint64_t seed, int site, void* o,
                              float* lse, void* stream);
int hct_attention_dropout_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, int B, int N, int H, int dh,
                              int dtype, float p, uint64_t seed, int site, void* dqkv, void* stream);
int hct_drop_path_scales(uint64_t seed, const int* sites, const float* rates, int n_sites, int B, float* out, void* stream);
int hct_residual_drop_apply(const void* x, int x_dtype, void* y, int y_dtype, const float* residual, int64_t B, int64_t seg,
                            const float* scales, uint64_t seed, int site, float p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Decoder input assembly (mae.py:257-265):
 *   y[b,0]   = e[b,0] + dec_cls
 *   y[b,1+l] = (ids_restore[b,l] < K ? e[b,1+ids_restore[b,l]] : mask_token) + dec_pos[l]
 * e [B,K+1,D] in e_dtype; y fp32 [B,L+1,D].
 * backward: de (e_dtype) gather of dy; dmask_token = sum over masked rows; ddec_cls = sum_b dy[b,0].
 * ------------------------------------------------------------------------------------------ */
int hct_decoder_assemble_fwd(const void* e, int e_dtype, const float* mask_token, const float* dec_cls,
                             const float* dec_pos, const int32_t* ids_restore, int B, int L, int K, int D,
                             float* y, void* stream);
int hct_decoder_assemble_bwd(const float* dy, const int32_t* ids_restore, const int32_t* ids_shuffle, int B,
                             int L, int K, int D, void* de, int de_dtype, float* dmask_token, float* ddec_cls,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Masked-voxel MSE (mae.py:277-301) fused with patchify (mae.py:160-170) and its backward seed.
 *   pred [B, L+1, pd] (row 0 of each volume = cls row, ignored; mae.py:273), pd = P^3*C (C fastest)
 *   loss (1 fp32, overwritten) = sum_l mask*mean_k (pred-tgt)^2 / sum(mask)
 *   dpred (may be NULL) same shape/dtype as pred: s*2*mask*(pred-tgt)/(pd*sum(mask)); 0 on cls/kept rows;
 *   s = *dpred_scale (device fp32, the incoming dLoss, e.g. a GradScaler factor) or 1 if NULL.
 *   loss may be NULL when only dpred is wanted.
 *   norm_pix: per-patch (t-mean)/sqrt(var_unbiased+1e-6) target (mae.py:290-293).
 *   mask_sum = sum(mask) (= B*(L-K) for masks from hct_mask_rank); row_loss: workspace of B*L floats.
 * ------------------------------------------------------------------------------------------ */
int hct_masked_mse(const void* pred, int pred_dtype, const void* x, int x_dtype /* HCT_F32 | HCT_F16 */, const float* mask, int B, int C, int S,
                   int P, int norm_pix, float mask_sum, float* row_loss, float* loss, void* dpred,
                   const float* dpred_scale, void* stream);
/* reconstructed voxels: unpatchify (mae.py:172-192). pred rows [B, L(+1 if has_cls_row), pd] -> [B,C,S,S,S] fp32 */
int hct_unpatchify(const void* pred, int pred_dtype, int has_cls_row, int B, int C, int S, int P, float* vol,
                   void* stream);

/* Feature-extraction input of the plain ViT encoder (src/models/vit.py:144-162): every patch is embedded, the class token
 * is prepended and the optional register tokens are inserted behind it:
 *   h[b,0,:] = cls;  h[b,1+r,:] = reg[r,:] (r < R);  h[b,1+R+l,:] = tok[b*L+l,:] + pos[l,:]        (pos / reg may be NULL) */
int hct_vit_assemble_fwd(const void* tok, int tok_dtype, const float* cls, const float* reg, const float* pos, int B,
                         int L, int R, int D, float* h, void* stream);

/* Classification heads over the ViT features, forward / eval-mode arithmetic (src/models/classifier.py:7-99 and the
 * `classification_head` of src/models/vit.py:133-137, :170-171).  All fp32 unless a dtype is given.
 *
 * hct_channel_norm: nn.BatchNorm1d(C, affine=False) in eval mode on [rows, C] (classifier.py:89 `bn1`):
 *   out[r, c] = (x[r, c] - mean[c]) / sqrt(var[c] + eps)                                   C % 4 == 0
 * hct_query_attention: the learnt queries of AttentionClassifier against every token (classifier.py:84-93):
 *   out[b, h, q, :] = softmax_n(logit_scale * <q[q, h*dh:(h+1)*dh], K[b, n, h, :]>) @ V[b, :, h, :]
 *   q: [Q, H*dh] fp32 (the raw `cls_token`; the reference scales it by `scale` and SDPA by dh^-1/2 again, so the caller
 *   passes logit_scale = scale * dh^-1/2); kv: [B, N, 2, H, dh] (the `wkv` output as it lies, classifier.py:90);
 *   out: [B, H, Q, dh] fp32 - the layout classifier.py:95 reshapes WITHOUT a permute.  Q*N + 4*Q*dh + Q <= 16384.
 * hct_head_linear: an optional eval-mode BatchNorm1d, the mean over nq consecutive D-vectors, a Linear and an optional Tanh:
 *   out[r, c] = act( sum_k (1/nq * sum_q (x[r*ldx + q*D + k] - mean[k]) / sqrt(var[k] + eps)) * W[c, k] + bias[c] )
 *   mean = var = NULL skips the normalisation; act = HCT_ACT_NONE | HCT_ACT_TANH.  (LinearClassifier: nq = 1, ldx = D;
 *   AttentionClassifier's bn2 + mean + linear: nq = Q, ldx = Q*D; ViT classification_head on x[:, 0]: ldx = T*D.) */
int hct_channel_norm(const float* x, const float* mean, const float* var, float eps, void* out, int out_dtype, int64_t rows,
                     int C, void* stream);
int hct_query_attention(const float* q, int Q, const void* kv, int kv_dtype, int B, int N, int H, int dh, float logit_scale,
                        float* out, void* stream);
int hct_head_linear(const float* x, int64_t ldx, int nq, const float* mean, const float* var, float eps, const float* W,
                    const float* bias, int act, float* out, int rows, int D, int n_out, void* stream);

/* Linear probing: LinearClassifier in TRAINING mode on frozen (detached) features with nn.CrossEntropyLoss
 * (main_downstream.py:142-146, :214; engine_downstream.py:70-117).  All fp32, fixed summation orders.
 *
 * hct_batchnorm_stats: nn.BatchNorm1d training statistics of x [B, D] (B > 1): mean[k], var[k] = biased variance (what the
 *   forward normalises with); if running_* are given: running = (1-momentum)*running + momentum*{mean, unbiased variance}.
 *   The forward itself is hct_head_linear with these mean / var.
 * hct_softmax_xent: loss = mean_b(logsumexp(logits[b]) - logits[b, target[b]]) (loss may be NULL);
 *   dlogits[b, c] = (softmax(logits[b])[c] - [c == target[b]]) * (dloss ? *dloss : 1) / B (dlogits may be NULL).
 * hct_head_linear_wgrad: dW[c, k] = sum_b dlogits[b, c] * (x[b, k] - mean[k]) / sqrt(var[k] + eps), db[c] = sum_b dlogits[b, c]
 *   (mean = var = NULL: no normalisation; db may be NULL).  The statistics are treated as constants: exact for the
 *   parameter gradients.  The gradient with respect to x is hct_bn_bwd_input (fine-tuning, below). */
int hct_batchnorm_stats(const float* x, int B, int D, float momentum, float* mean, float* var, float* running_mean,
                        float* running_var, void* stream);
int hct_softmax_xent(const float* logits, const int64_t* target, int B, int n_classes, const float* dloss, float* loss,
                     float* dlogits, void* stream);
int hct_head_linear_wgrad(const float* x, const float* mean, const float* var, float eps, const float* dlogits, int B, int D,
                          int n_out, float* dW, float* db, void* stream);

/* Multi-label fine-tuning (TRAIN.LABEL_NAMES): sigmoid + binary cross-entropy over a table of T labels per scan with gaps.  An
 * addition of this build -- the reference trains one binary model per label (main_downstream.py:214) and has no such loss; the
 * value is torch's binary_cross_entropy_with_logits(x, y, weight = valid, pos_weight = w, reduction = 'sum') / max(n, 1).
 *   logits, target: fp32 [B, T] row-major.  target[b, t] in [0, 1] is the label (it may be soft); target[b, t] < 0 (or NaN)
 *   marks the entry as missing.  pos_weight: [T], NULL = 1.  dloss: device scalar g multiplying the gradient, NULL = 1.
 *   loss (1 float), label_loss [T] and dlogits [B, T] may each be NULL, but not all three.
 * With n = the number of valid entries, w = pos_weight[t], y = target[b, t], x = logits[b, t], s = the logistic function:
 *   l(x, y, w)    = (1 - y) x + (1 + (w - 1) y) softplus(-x),  softplus(-x) = max(-x, 0) + log1p(exp(-|x|)),
 *                   evaluated as (1 - y) softplus(x) + w y softplus(-x): the same value, without cancellation at x < 0;
 *   loss          = sum of l over the valid entries / max(n, 1);
 *   label_loss[t] = mean of l over the valid rows of column t, 0 where the column has none;
 *   dlogits[b, t] = g ((1 - y) s(x) - w y s(-x)) / max(n, 1) for a valid entry (s(x) and s(-x) both from exp(-|x|), neither as
 *                   one minus the other), exactly 0.0f for a missing one.
 * n = 0: the loss is 0 and every gradient is 0 (torch's mean over no element is NaN there).
 * Any B, T >= 1.  Fixed summation order, no floating-point atomics: two identical calls agree bit for bit.  The workspace
 * (hct_sigmoid_bce_workspace_bytes, 8-byte aligned) holds the per-row-block partial sums and the count; too small a one gives
 * HCT_E_WORKSPACE, bad arguments HCT_E_BADARG, and no output is touched in either case. */
size_t hct_sigmoid_bce_workspace_bytes(int B, int T);
int hct_sigmoid_bce(const float* logits, const float* target, const float* pos_weight, int B, int T, const float* dloss, float* loss,
                    float* label_loss, float* dlogits, void* workspace, size_t workspace_bytes, void* stream);

/* Mixup, CutMix and label smoothing of the fine-tuning recipe (TRAIN.MIXUP / CUTMIX / LABEL_SMOOTHING).  Additions of this build:
 * the reference trains on plain batches with nn.CrossEntropyLoss (main_downstream.py:214).  Sample b is always mixed with its
 * partner p = B - 1 - b (timm's x.flip(0)); the two members of a pair are independent, each with its own lam and its own box.
 *
 * hct_mix_volumes: x fp32 [B, C, S, S, S], contiguous, 16-byte aligned, mixed IN PLACE in one launch and one pass: the thread that
 *   owns a voxel of a pair loads both members, computes both and stores both (8 bytes per voxel moved).
 *   lam [B] device fp32;  box [B, 6] device int32 (lo0, hi0, lo1, hi1, lo2, hi2), axis 0 slowest, half-open, or NULL = no boxes.
 *   With x0 the contents before the call: sample b has a box when box != NULL and lo < hi on all three axes after each bound is
 *   clamped to [0, S] (the table lives on the device, so its values cannot be refused here).  Then x[b, c, v] = x0[p, c, v] inside
 *   the box and x0[b, c, v] outside, both bit copies, and lam[b] is not used for voxels.  Otherwise
 *   x[b, c, v] = fma(lam[b], x0[b, c, v], (1 - lam[b]) * x0[p, c, v]) in fp32.  p == b (the middle sample of an odd batch) stays
 *   bit-unchanged, as does every voxel no box reaches and every sample that mixes with lam == 1 (neither is loaded or stored):
 *   lam == 1 is the exact identity whatever the partner holds, where the formula would give NaN against an Inf or NaN partner.
 *   S % 4 == 0, S <= 1024, B * C <= 65535 (the limits of hct_gather_augment); anything else, a null x or lam, or a misaligned x
 *   returns HCT_E_BADARG before any launch and touches nothing.
 * hct_mix_xent: soft-target cross-entropy whose target is never materialised.  logits fp32 [B, n_classes], target int64 [B]
 *   (compared with the class index only, never used as one), lam [B] device fp32 or NULL, 0 <= smoothing < 1.  With
 *   s(y)[c] = (1 - smoothing) [c == y] + smoothing / n_classes:
 *     t[b, c]       = lam[b] s(target[b])[c] + (1 - lam[b]) s(target[p])[c]   (lam == NULL: s(target[b])[c]);
 *     loss          = 1/B sum_b sum_c t[b, c] (logsumexp(logits[b]) - logits[b, c])   (loss may be NULL);
 *     dlogits[b, c] = (softmax(logits[b])[c] - t[b, c]) * (dloss ? *dloss : 1) / B   (dlogits may be NULL; not both).
 *   Any B, n_classes >= 1.  One launch of one workgroup, max-subtracted exponentials, fixed summation order, no floating-point
 *   atomics: two identical calls agree bit for bit.  Bad arguments (smoothing outside [0, 1) among them) return HCT_E_BADARG and
 *   touch nothing. */
int hct_mix_volumes(float* x, int B, int C, int S, const float* lam, const int32_t* box, void* stream);
int hct_mix_xent(const float* logits, const int64_t* target, const float* lam, float smoothing, int B, int n_classes, const float* dloss,
                 float* loss, float* dlogits, void* stream);

/* Fine-tuning through the heads (engine_downstream.py:70-117 with TRAIN.LOCK False: the backbone trains through the head).
 * Fixed summation orders, no floating-point atomics: two identical calls give bit-identical results.  x_dtype / kv_dtype:
 * HCT_F32 or HCT_BF16 (the backbone's output read as it lies); everything else fp32.
 *
 * hct_bn_stats_rows: hct_batchnorm_stats over many rows of x [rows, D] (row stride ldx): per chunk of 128 rows the chunk's mean
 *   and sum of squared deviations, merged over the chunks in index order (rows <= 128: bit-identical to hct_batchnorm_stats).
 *   workspace >= hct_bn_rows_workspace_bytes(rows, D).
 * hct_bn_norm: out[r, k] = (x[r*ldx + k] - mean[k]) / sqrt(var[k] + eps) into a dense [rows, D] (D, ldx multiples of 4).
 * hct_bn_bwd_input: BatchNorm1d(affine=False) training backward with respect to its input, batch statistics mean / var:
 *   dx[r*ldo + k] = rstd * (g - mean_r g - xhat * mean_r(g * xhat)),  xhat = (x - mean) * rstd,  rstd = 1 / sqrt(var + eps)
 *   g [rows, D] (row stride ldg), or g == NULL and the dgrad of the Linear that follows the norm is fused in:
 *   g[r, k] = 1/nq * sum_c dlogits[r / nq, c] * W[c, k]  (LinearClassifier: nq = 1; AttentionClassifier's bn2 + mean over the
 *   queries: nq = Q).  dx in dx_dtype.  workspace >= hct_bn_rows_workspace_bytes(rows, D) + 2 * D * 4.
 * hct_head_linear_x: hct_head_linear (act none) with x in x_dtype.
 * hct_head_linear_bwd: hct_head_linear_wgrad generalised to x_dtype, a row stride ldx and the mean over nq consecutive
 *   D-vectors: dW[c, k] = sum_b dlogits[b, c] * 1/nq * sum_q xhat[b*ldx + q*D + k],  db[c] = sum_b dlogits[b, c].
 * hct_query_attention_lse: hct_query_attention that also writes lse [B, H, Q] = the log-sum-exp of each softmax row.
 * hct_query_attention_bwd: its backward from dout [B, H, Q, dh] fp32, P recomputed from lse: dkv [B, N, 2, H, dh] in kv_dtype
 *   (every key / value row read once and written once), dq [Q, H*dh] = the cls_token gradient summed over the batch in batch
 *   order, logit_scale included.  dh <= 128, 6*Q*dh + 2*Q <= 16384.  workspace >= hct_query_attention_bwd_workspace_bytes.
 * hct_clip_total_norm: torch.nn.utils.clip_grad_norm_ on a flat gradient buffer from its per-segment L2 norms (hct_grad_norms
 *   with clip 0): nrm[0] = sqrt(sum norms^2), nrm[1] = min(1, max_norm / (nrm[0] + 1e-6)); grads *= nrm[1] (total % 4 == 0).
 * hct_add_f32: dst[i] += src[i] (a head's gradients accumulated into its flat buffer; n % 4 == 0). */
size_t hct_bn_rows_workspace_bytes(int rows, int D);
int hct_bn_stats_rows(const void* x, int x_dtype, int64_t ldx, int rows, int D, float momentum, float* mean, float* var,
                      float* running_mean, float* running_var, void* workspace, size_t workspace_bytes, void* stream);
int hct_bn_norm(const void* x, int x_dtype, int64_t ldx, int64_t rows, int D, const float* mean, const float* var, float eps,
                void* out, int out_dtype, void* stream);
int hct_bn_bwd_input(const void* x, int x_dtype, int64_t ldx, const float* mean, const float* var, float eps, const float* g,
                     int64_t ldg, const float* dlogits, const float* W, int nq, int n_classes, int rows, int D, void* dx,
                     int dx_dtype, int64_t ldo, void* workspace, size_t workspace_bytes, void* stream);
int hct_head_linear_x(const void* x, int x_dtype, int64_t ldx, int nq, const float* mean, const float* var, float eps,
                      const float* W, const float* bias, float* out, int rows, int D, int n_out, void* stream);
int hct_head_linear_bwd(const void* x, int x_dtype, int64_t ldx, int nq, const float* mean, const float* var, float eps,
                        const float* dlogits, int B, int D, int n_out, float* dW, float* db, void* stream);
int hct_query_attention_lse(const float* q, int Q, const void* kv, int kv_dtype, int B, int N, int H, int dh, float logit_scale,
                            float* out, float* lse, void* stream);
size_t hct_query_attention_bwd_workspace_bytes(int B, int Q, int H, int dh);
int hct_query_attention_bwd(const float* q, int Q, const void* kv, int kv_dtype, int B, int N, int H, int dh, float logit_scale,
                            const float* out, const float* lse, const float* dout, void* dkv, float* dq, void* workspace,
                            size_t workspace_bytes, void* stream);
int hct_clip_total_norm(float* grads, int64_t total, const float* norms, int nseg, float max_norm, float* nrm, void* stream);
int hct_add_f32(float* dst, const float* src, int64_t n, void* stream);

/* Device side of the reference's per-sample MAE input transforms, mae3d_transforms(mode='train'), src/data/transforms.py:
 * 193-228: CastToTyped(float32) of the cached volume (fp16 on disk, transforms.py:170-175) -> RandFlipd on spatial axes
 * 0, 1, 2 -> RandShiftIntensityd.  The random draws stay on the host (one byte of flip flags and one offset per sample);
 *   out[b, c, i, j, k] = (float)in[b, c, f0(i), f1(j), f2(k)] + shift[b],   f_a(t) = S-1-t if flip[b] bit a else t.
 * in: [B, C, S, S, S] of in_dtype (HCT_F16 / HCT_BF16 / HCT_F32), out fp32 (may not alias in).  flip / shift may be NULL.
 * RandGaussianSmoothd (transforms.py:230-238) is not part of this call. */
/* ------------------------------------------------------------------------------------------
 * DINO self-distillation (BASELINE config #5; reference engine_pretrain_dino.py:14-130).
 *   hct_dino_loss: DINOLoss.forward, src/losses/losses.py:63-91, plus the gradient w.r.t. the student logits and the column
 *     sums of the teacher logits that update_center (:93-102) all-reduces.  student [V*B, K] (crop-major: row v*B + b),
 *     teacher [2*B, K], both `dtype`; center [K] fp32; loss: 1 device fp32.  dstudent (same shape / dtype as student) and
 *     batch_center_sum [K] may be NULL; dloss: device scalar multiplying the gradient, or NULL for 1.
 *   hct_dino_center_update: center = center * momentum + (batch_center_sum / count) * (1 - momentum), count = 2*B*world.
 *   hct_ema_update: momentum encoder, src/utils/misc.py:386-397: k = k * m + (1 - m) * q over a flat fp32 buffer.
 * ------------------------------------------------------------------------------------------ */
size_t hct_dino_loss_workspace_bytes(int n_crops, int B, int K);
int hct_dino_loss(const void* student, const void* teacher, int dtype, int n_crops, int B, int K, const float* center, float student_temp,
                  float teacher_temp, float* loss, void* dstudent, const float* dloss, float* batch_center_sum, void* workspace,
                  size_t workspace_bytes, void* stream);
int hct_dino_center_update(float* center, const float* batch_center_sum, int K, double momentum, double count, void* stream);
int hct_ema_update(float* momentum_params, const float* params, int64_t n, double m, void* stream);
/* Sinkhorn-Knopp teacher (DINOv2 sinkhorn_knopp_teacher) in the log domain: q[b,k] = exp(t[b,k] / T + lr[b] + lc[k] + log N), N = rows of all
 * ranks, with lc[k] = -log K - logsumexp_b(t[b,k] / T + lr[b]) over all ranks' rows and lr[b] = -log N - logsumexp_k(t[b,k] / T + lc[k]),
 * alternating from lr = 0.  teacher [R, K] of `dtype` (fp32 / bf16), K % 4 == 0.
 *   hct_dino_sk_col_lse: out[k] = logsumexp over this rank's R rows of t[b,k] * inv_temp + lr[b] (lr NULL: zeros); the caller combines the
 *     ranks and forms lc.  Workspace: hct_dino_sk_workspace_bytes(R, K).
 *   hct_dino_sk_row_lse: out[b] = logsumexp over k of t[b,k] * inv_temp + lc[k].
 *   hct_dino_loss_sk: hct_dino_loss with the teacher distribution given by (lc [K], lr [2B], log_n = log N) in the place of (center, the
 *     teacher's own row statistics); same loss, dstudent and dloss, no centre sums.  Workspace: hct_dino_loss_sk_workspace_bytes. */
size_t hct_dino_sk_workspace_bytes(int R, int K);
int hct_dino_sk_col_lse(const void* teacher, int dtype, int R, int K, float inv_temp, const float* lr, float* out, void* workspace,
                        size_t workspace_bytes, void* stream);
int hct_dino_sk_row_lse(const void* teacher, int dtype, int R, int K, float inv_temp, const float* lc, float* out, void* stream);
size_t hct_dino_loss_sk_workspace_bytes(int n_crops, int B, int K);
int hct_dino_loss_sk(const void* student, const void* teacher, int dtype, int n_crops, int B, int K, const float* lc, const float* lr, float log_n,
                     float student_temp, float teacher_temp, float* loss, void* dstudent, const float* dloss, void* workspace,
                     size_t workspace_bytes, void* stream);
/* iBOT masked patch-token loss (DINOv2 iBOTPatchLoss.forward_masked): student row i is paired with teacher row i, M rows of K
 * prototypes, both of `dtype` (fp32 / bf16), K % 4 == 0, any M >= 1; weight [M] fp32 (1 / masked patches of the row's image);
 * inv_images = 1 / n_g (global crops of this rank).
 *   q_i   = softmax((t_i - center) / T_t)                         (hct_ibot_loss)
 *   q_i   = exp(t_i / T_t + lr[i] + lc + log_n)                    (hct_ibot_loss_sk; lc [K], lr [M], log_n = log of the masked rows of all ranks)
 *   loss  = -inv_images * sum_i w_i sum_k q_ik log_softmax(s_i / T_s)_k
 *   ds_ik = dloss * w_i * inv_images / T_s * (softmax(s_i / T_s)_k - q_ik)          (dloss: device scalar, or NULL for 1)
 *   center_sum[k] = sum_i t_ik                                      (hct_ibot_loss only)
 * dstudent and center_sum may be NULL.  student / dstudent are plain pointers to M contiguous rows, so they may be the tail rows of a
 * larger [rows, K] buffer.  Every logit is read twice (row statistics, then loss + gradient).  Blocks of the second pass own a
 * 1024-column chunk of 64 consecutive rows and walk them in row order; the loss partials and the centre partials of the row splits
 * are folded in a fixed order, so a call is repeatable bit for bit.  A workspace shorter than hct_ibot_loss_workspace_bytes is refused
 * before anything is launched. */
size_t hct_ibot_loss_workspace_bytes(int M, int K);
int hct_ibot_loss(const void* student, const void* teacher, int dtype, int M, int K, const float* weight, const float* center, float student_temp,
                  float teacher_temp, float inv_images, float* loss, void* dstudent, const float* dloss, float* center_sum, void* workspace,
                  size_t workspace_bytes, void* stream);
int hct_ibot_loss_sk(const void* student, const void* teacher, int dtype, int M, int K, const float* weight, const float* lc, const float* lr,
                     float log_n, float student_temp, float teacher_temp, float inv_images, float* loss, void* dstudent, const float* dloss,
                     void* workspace, size_t workspace_bytes, void* stream);
/* KoLeo regulariser (DINOv2 KoLeoLoss) on n >= 2 feature rows x [n, D] of `dtype` (fp32 / bf16) read with row stride ldx (elements; D % 4 == 0,
 * D <= 4096, ldx % 4 == 0): xh = x / max(||x||, 1e-8), nn_index[i] = argmax_{j != i} xh_i . xh_j (lowest index on ties),
 * dist[i] = ||xh_i - xh_nn + 1e-8||, loss = -mean log(dist + 1e-8); inv_norm[i] = 1 / max(||x_i||, 1e-8).  fp32 arithmetic.
 *   hct_koleo_bwd: dx (dtype of x, row stride lddx) = dloss * d loss / d x with nn_index held constant; dloss: device scalar, or NULL for 1.
 *     Every row gathers the rows that chose it in row order (no atomics). */
int hct_koleo_fwd(const void* x, int dtype, int n, int D, int64_t ldx, float* loss, int32_t* nn_index, float* dist, float* inv_norm, void* stream);
int hct_koleo_bwd(const void* x, int dtype, int n, int D, int64_t ldx, const int32_t* nn_index, const float* dist, const float* inv_norm,
                  const float* dloss, void* dx, int64_t lddx, void* stream);
/* DINOHead tail (src/models/dino_head.py:37-41): rows L2-normalised (F.normalize, eps 1e-12), prototype weights weight-normalised
 * (torch.nn.utils.weight_norm, dim 0: W[k,:] = g[k] v[k,:] / ||v[k,:]||); forward keeps 1 / norm per row for the backward. */
int hct_l2norm_rows_fwd(const float* z, int M, int n, void* zn, int zn_dtype, float* inv_norm, void* stream);
/* Projection head with use_bn (dino_head.py:15-21, the default of config.py:86): Linear -> BatchNorm1d -> GELU.  u [M, D] fp32 is the
 * Linear's output, mean / var [D] the statistics to normalise with -- hct_batchnorm_stats of u in training (the caller all-reduces
 * them under data parallelism, as the SyncBatchNorm of main_pretrain_dino.py:183-185 does), the running ones in eval:
 *   fwd   : xhat = (u - mean) / sqrt(var + eps); h = gelu(gamma * xhat + beta) in h_dtype; xhat and dact = gelu'(.) fp32 kept for the
 *           backward (either may be NULL)
 *   sums  : sums[0..D) = sum_rows dh * dact (= dbeta), sums[D..2D) = sum_rows dh * dact * xhat (= dgamma) of this rank's rows
 *   apply : du = gamma / sqrt(var + eps) * (dh * dact - sums[0] / count - xhat * sums[1] / count), count = rows that shared the
 *           statistics (all ranks; `sums` all-reduced then), du in dh's dtype or fp32                                          */
int hct_bn_gelu_fwd(const float* u, const float* mean, const float* var, const float* gamma, const float* beta, float eps, int M, int D, void* h,
                    int h_dtype, float* xhat, float* dact, void* stream);
int hct_bn_gelu_bwd_sums(const void* dh, int dh_dtype, const float* dact, const float* xhat, int M, int D, float* sums, void* stream);
int hct_bn_gelu_bwd_apply(const void* dh, int dh_dtype, const float* dact, const float* xhat, const float* gamma, const float* var, float eps,
                          const float* sums, double count, int M, int D, void* du, int du_dtype, void* stream);
int hct_l2norm_rows_bwd(const float* dzn, const void* zn, int zn_dtype, const float* inv_norm, int M, int n, float* dz, void* stream);
int hct_weight_norm_fwd(const float* v, const float* g, int K, int n, void* w, int w_dtype, float* inv_norm, void* stream);
int hct_weight_norm_bwd(const float* dw, const float* v, const float* g, const float* inv_norm, int K, int n, float* dv, float* dg /* or NULL */,
                        void* stream);

/* HU windowing of loading_transforms (src/data/transforms.py:108-133): ScaleIntensityRanged(a_min, a_max, 0, 1, clip) for one
 * channel (window 40 +- 150), MultipleWindowScaleStack (transforms.py:8-36) for three ((40,80), (80,200), (600,2800) as
 * centre, width -> a_min = l - w/2, a_max = l + w/2), stacked on the channel axis:
 *   out[b, w, v] = clip((hu[b, v] - a_min[w]) / (a_max[w] - a_min[w]), 0, 1),   hu [B, voxels] -> out [B, n_windows, voxels].
 * in / out dtype HCT_F32 or HCT_F16 (fp16 = the persistent cache's type, transforms.py:171-178); a_min / a_max device fp32. */
int hct_hu_window(const void* hu, int in_dtype, void* out, int out_dtype, int B, int64_t voxels, int n_windows, const float* a_min,
                  const float* a_max, void* stream);
int hct_augment_volume(const void* in, int in_dtype, float* out, int B, int C, int S, const unsigned char* flip,
                       const float* shift, void* stream);
/* RandGaussianSmoothd of mae3d_transforms(reshape=False) (src/data/transforms.py:230-238; MONAI GaussianSmooth ->
 * GaussianFilter -> separable_filtering with zero padding): in [B,C,S,S,S] fp32 -> out, one 1-D pass per spatial axis.
 *   taps  [B][3][9] device fp32: sample b's centred kernel of spatial axis a (0 = slowest), zero beyond its tail; the host
 *         computes them as MONAI's gaussian_1d(sigma, truncated=4, approx="erf") does (sigma <= 1.06 keeps 9 taps);
 *   apply [B] device bytes: 0 = the transform did not fire for this sample (out = in).
 * tmp: scratch of the same size as in/out; the three buffers must differ. */
int hct_gaussian_smooth3d(const float* in, float* out, float* tmp, int B, int C, int S, const float* taps, const unsigned char* apply,
                          void* stream);

/* DINO multi-crop augmentation, DataAugmentationDINO3D (src/data/transforms.py:39-105), resampling part: CastToType(float32) ->
 * ResizeWithPadOrCrop -> [CenterSpatialCrop] -> RandSpatialCrop -> Resize(mode "area") -> RandFlip x 3 -> RandShiftIntensity,
 * for every view of a batch in one launch and one pass (no padded field, no intermediate crop is written).
 *   in    [B, C, S, S, S] HCT_F16 / HCT_BF16 / HCT_F32;  out [n_views, B, C, F, F, F] fp32 contiguous (out[v] is a ready crop)
 *   boxes [n_views, B, 6] device int32: start[3], size[3] of the box IN INPUT-VOLUME COORDINATES, signed: whatever lies outside
 *         [0, S) reads as zero, so padding, centre crop and the fields are the host's arithmetic; 1 <= size (<= 65536)
 *   area resize: resized index i along an axis of n box voxels averages box voxels [floor(i n / F), ceil((i + 1) n / F))
 *         (= adaptive average pooling = F.interpolate(mode="area")); the sum runs over the voxels inside the volume in ascending
 *         x, y, z order (fixed: two calls are bit-identical) and is divided by the full window's voxel count
 *   flip  [n_views, B] device bytes or NULL: bit a = spatial axis a (0 = slowest) of the RESIZED crop is mirrored
 *   shift [n_views, B] device fp32 or NULL: added after the divide
 * F % 4 == 0 (a thread stores 4 outputs as 16 bytes), F <= 2044 (a volume's F^3 / 4 threads, rounded up to whole blocks, are
 * counted in an int; a larger F is refused); n_views * B * C <= 65535; outputs whose window lies wholly outside the
 * volume issue no loads. */
int hct_crop_resize_area(const void* in, int in_dtype, int B, int C, int S, float* out, int F, int n_views, const int32_t* boxes,
                         const unsigned char* flip, const float* shift, void* stream);
/* RandAdjustContrast of the second global crop (MONAI AdjustContrast), in place on x [B, n] fp32 (n = C F^3, n % 4 == 0):
 *   mn, mx = min, max over the whole sample;  x = ((x - mn) / (mx - mn + 1e-7)) ** gamma[b] * (mx - mn) + mn    (fp32, powf)
 * Two launches: per-sample partial min / max over a (chunks, B) grid into the workspace (no floating-point atomics; min / max do
 * not depend on the order, so the result is exact), then the pointwise pass, which folds its sample's partials first.
 *   gamma [B] device fp32;  apply [B] device bytes: samples with 0 stay bit-identical
 *   workspace >= hct_adjust_contrast_workspace_bytes(B, n) */
size_t hct_adjust_contrast_workspace_bytes(int B, int64_t n);
int hct_adjust_contrast(float* x, int B, int64_t n, const float* gamma, const unsigned char* apply, void* workspace, size_t workspace_bytes,
                        void* stream);

/* Batch assembly of the fine-tuning loader out of a device-resident pool of cache items: gather by slot index, then the
 * arithmetic of hct_augment_volume (vit_transforms, src/data/transforms.py:258-320: cast to fp32, three axis flips, intensity
 * shift), in one launch and one pass; the gathered fp16 batch is never written.
 *   pool  [n_slots, C, S, S, S] fp16 (never written);  out [B, C, S, S, S] fp32
 *   slot  [B] device int32: out[b] is made of pool[slot[b]]; -1 = the all-zero placeholder volume, through the same arithmetic.
 *         The table lives on the device, so a value outside [-1, n_slots) cannot be refused here: the kernel reads nothing for
 *         it and treats it as -1 (callers that hold the indices on the host check them there)
 *   flip  [B] device bytes or NULL: bit a = spatial axis a (0 = slowest) is mirrored;  shift [B] device fp32 or NULL: added
 *         after the cast.  Both NULL = the plain widening gather of validation and test.
 * S % 4 == 0, B * C <= 65535, out 16-byte aligned.  S % 8 == 0 with a 16-byte aligned pool takes 16-byte loads and stores,
 * otherwise 8-byte loads.  Timed as class 7 of the measurement hooks with 2 bytes read + 4 written per voxel. */
int hct_gather_augment(const void* pool, const int32_t* slot, float* out, int B, int C, int S, int64_t n_slots, const unsigned char* flip,
                       const float* shift, void* stream);

/* Random 3-D affine augmentation of the fine-tuning recipe (TRAIN.AFFINE_*; MONAI's RandAffine, an addition of this build: the
 * reference's vit_transforms has flips and the shift only).  The whole train-time transform of a batch in one launch and one pass:
 * gather, affine resampling with trilinear interpolation, shift, widening to fp32.
 *   in    slot != NULL: the pool [n_slots, C, S, S, S], HCT_F16, with the slot semantics of hct_gather_augment (-1 or out of
 *         range = the all-zero volume, nothing is read for it).  slot == NULL: a stacked batch [B, C, S, S, S] in HCT_F16 /
 *         HCT_BF16 / HCT_F32 (n_slots is not looked at).  Never written.   out [B, C, S, S, S] fp32, may not alias in.
 *   mat   [B, 12] device fp32 or NULL: the rows of [A | t] in voxel units, the map from OUTPUT to INPUT coordinates about the
 *         volume centre c = (S - 1) / 2.  For output index i = (i0, i1, i2), axis 0 slowest, p = i - c (exact) and, per axis a,
 *           q_a = fma(A_a2, p_2, fma(A_a1, p_1, fma(A_a0, p_0, t_a + c)))
 *         in fp32: one rounding for t_a + c and one per fused multiply-add, four in all.
 *   sampling: trilinear from the eight voxels around q.  Per axis f = floor(q), w1 = q - f, w0 = 1 - w1; the weight of tap
 *         (d0, d1, d2) is (w_d0 * w_d1) * w_d2 (two roundings); the sum is acc = fma(w, v, acc) from acc = 0 over the taps in
 *         ascending (d0, d1, d2), d2 fastest (a rounding per tap); out = acc + shift[b] (one more).  A tap outside [0, S) on any
 *         axis has the VALUE zero (not a zero weight: a neighbouring Inf stays out of it) and is not loaded: grid_sample's
 *         padding_mode="zeros" with align_corners=True.
 *         Whether a tap is inside is decided on the floating-point coordinate, `q > -1 && q < S`, before any conversion to an
 *         integer; a NaN fails it.  Only a coordinate that passed is converted (0 stands in for one that failed), and every voxel
 *         index a load uses is clamped to [0, S - 1] per axis ([0, S - 2] for the contiguous axis, whose two taps are one load of
 *         two adjacent voxels) and added to the base pointer of the sample's own channel: whatever `mat` holds -- huge, infinite or
 *         NaN values included -- no address outside the sample's own C volumes can be produced.  What a lane loads in place of a
 *         tap that is outside is a voxel of that same volume, and it is discarded.  (The table lives on the device, so it cannot be
 *         refused here; a sample mapped wholly outside is exactly shift[b] everywhere.)
 *   fire  [B] device bytes or NULL (= every sample fires).  Where fire[b] == 0 the sample takes the arithmetic of
 *         hct_gather_augment / hct_augment_volume bit for bit -- out = (float)in[flips(i)] + shift[b] with flip[b]'s bits -- and
 *         mat[b] is not read.  Where it fires, the host has folded the flips into A and flip[b] is ignored.  The choice is
 *         uniform per workgroup: a workgroup never spans two samples.
 *   flip  [B] device bytes or NULL;  shift [B] device fp32 or NULL: added after the interpolation.
 *   mat == NULL requires fire == NULL and makes the call hct_gather_augment (slot != NULL) or hct_augment_volume (slot == NULL).
 * The channels of a sample share coordinates and weights: they are computed once per output voxel.  Fixed order, no atomics: two
 * identical calls agree bit for bit.
 * Limits: S % 4 == 0 (a thread stores 4 outputs as 16 bytes), S <= 1024, B * C <= 65535, out 16-byte aligned, in 8-byte aligned
 * (16-byte for HCT_F32; the paired taps are 4-byte loads at 2-byte alignment), a pool HCT_F16 with n_slots >= 1.  Anything else, a null in or out, or fire without mat returns
 * HCT_E_BADARG before any launch, with hct_last_error_string set, and touches nothing.
 * Timed as class 7 of the measurement hooks (the loader class) with 2 bytes read + 4 written per voxel as the floor. */
int hct_affine_augment(const void* in, int in_dtype, const int32_t* slot, int64_t n_slots, float* out, int B, int C, int S, const float* mat,
                       const unsigned char* fire, const unsigned char* flip, const float* shift, void* stream);

/* hct_affine_labels (csrc/affine.hip): the label volumes of a segmentation batch through the table hct_affine_augment takes for the
 * scans (an addition of this build; MONAI's RandAffined(mode=("bilinear", "nearest"))).  One launch: gather by slot, nearest
 * neighbour, a caller-chosen byte outside.
 *   pool  [n_slots, S, S, S] uint8, slot [B] device int32 with the semantics of hct_gather_flip_labels: a slot outside
 *         [0, n_slots) -- -1 by contract -- reads nothing and gives an all-255 volume, whatever mat, fire and outside hold.
 *   out   [B, S, S, S] uint8, may not be the pool.
 *   mat   [B, 12] device fp32 or NULL: the SAME table, flips folded in.  q_a is computed by the very expression above (one device
 *         function serves both kernels).  n_a = floor(q_a + 0.5): the nearest voxel, a tie q_a = n + 0.5 going to n + 1.  (Taken
 *         as floor(q) + (q - floor(q) >= 0.5), which is exact on the fp32 q; q + 0.5f itself would round.)  An axis is inside iff
 *         q_a >= -0.5 && q_a < S - 0.5, decided on the float before any conversion, in a form a NaN fails: q = -0.5 is voxel 0,
 *         q = S - 0.5 is outside.  out = pool[slot][n_0, n_1, n_2] where the three axes are inside, else `outside`.  The load is
 *         made from an address clamped into the sample's own volume, and the value selected afterwards: whatever mat holds, no
 *         address leaves that volume.  Label bytes are opaque: 255 travels like any other value.
 *   fire  [B] device bytes or NULL (= every sample fires).  Where fire[b] == 0 the sample is flips(pool[slot[b]]) with flip[b]'s
 *         bits, as hct_gather_flip_labels copies it, and mat[b] is not read; where it fires flip[b] is ignored.
 *   mat == NULL requires fire == NULL and makes the call hct_gather_flip_labels.
 * Limits: S % 4 == 0 (a thread stores 4 labels as one word), S <= 1024, B <= 65535, n_slots >= 1, both pointers 4-byte aligned.
 * Anything else, a null pool, slot or out, out == pool, or fire without mat returns HCT_E_BADARG before any launch. */
int hct_affine_labels(const uint8_t* pool, const int32_t* slot, int64_t n_slots, uint8_t* out, int B, int S, const float* mat,
                      const unsigned char* fire, const unsigned char* flip, uint8_t outside, void* stream);

/* Loading chain of loading_transforms (src/data/transforms.py:108-178) for ONE decoded volume: Orientationd("RAS") ->
 * Spacingd(1 mm, mode=3) -> CropForegroundd -> windowing -> Resized(roi) -> CastToTyped(fp16).  Four calls on one stream; none
 * waits for the host (shapes come from the file header, the foreground box stays in device memory).
 *
 * hct_volume_to_ras: raw voxels of the file (NIfTI-1 datatype code 2 uint8, 4 int16, 8 int32, 16 float32, 64 float64, 256 int8,
 *   512 uint16; native byte order; file order, axis i of ni voxels contiguous) -> out fp32 [d0, d1, d2], d[o] = n[perm[o]]:
 *   output axis o is file axis perm[o], reversed where flip[o] (host arrays of 3).  value = (float)((double)raw * slope + inter)
 *   where `scaled`, else (float)raw.
 * hct_bspline3_resample: in [n0, n1, n2] -> out [m0, m1, m2] fp32, every axis 1 ... 1024, as three 1-D passes (axis 0, 1, 2):
 *     out[j] = sum_{t < 32} weights[t][j] * in[clamp(base[j] + t, 0, n - 1)]        (ascending t, fused multiply-add)
 *   in float64 (weights, sums and the two intermediate volumes, which live in the workspace), rounded to fp32 once at the end, as
 *   MONAI's Spacing computes in float64 and casts.  base: device int32, the tables of the three axes one after the other
 *   [m0 + m1 + m2]; weights: device float64, per axis [32][m_axis], one after the other.  With the tables of headct_foundation_amd.nifti.bspline3_tables this is
 *   scipy.ndimage.map_coordinates(order=3, mode="nearest") at the coordinates j * step per axis.
 * hct_foreground_bbox: box[6] = start[3], size[3] of the voxels > 0 of vol [m0, m1, m2]; status[0] = 0, or
 *   HCT_LOAD_EMPTY_FOREGROUND where there is none (box = the whole volume then).  Both device int32.
 * hct_crop_window_resize_area: out[c, i, j, k] (fp16 [n_windows, R0, R1, R2]) = mean over the box voxels of bin (i, j, k) of
 *   clip((v - a_min[c]) / (a_max[c] - a_min[c]), 0, 1); the bin of index i on an axis of box length n is [floor(i n / R),
 *   ceil((i + 1) n / R)) (adaptive average pooling = F.interpolate(mode="area")); sums in ascending x, y, z.  box: device
 *   int32[6] (as hct_foreground_bbox writes it; confined to the volume by the kernel); a_min / a_max device fp32; 1 ... 4 windows;
 *   any R, 16-byte stores where R2 % 8 == 0. */
#define HCT_LOAD_EMPTY_FOREGROUND 1
int hct_volume_to_ras(const void* raw, int nifti_datatype, int ni, int nj, int nk, const int* perm, const int* flip, int scaled, double slope,
                      double inter, float* out, void* stream);
size_t hct_bspline3_resample_workspace_bytes(int n0, int n1, int n2, int m0, int m1, int m2);
int hct_bspline3_resample(const float* in, int n0, int n1, int n2, float* out, int m0, int m1, int m2, const int32_t* base, const double* weights,
                          void* workspace, size_t workspace_bytes, void* stream);
size_t hct_foreground_bbox_workspace_bytes(int m0, int m1, int m2);
int hct_foreground_bbox(const float* vol, int m0, int m1, int m2, int32_t* box, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int hct_crop_window_resize_area(const float* vol, int m0, int m1, int m2, const int32_t* box, int n_windows, const float* a_min, const float* a_max,
                                void* out, int R0, int R1, int R2, void* stream);

/* Resume at another resolution: trilinear resize (align_corners = false) of the learnable position table
 * src [extra + g_src^3, D] -> dst [extra + g_dst^3, D], the `extra` leading (class) rows copied unchanged.
 * Replaces interpolate_pos_embed's 3-D branch, src/utils/pos_embed.py:102-153 (called at main_pretrain_mae.py:132). */
int hct_pos_embed_interp3d(const float* src, int g_src, float* dst, int g_dst, int D, int extra, void* stream);

/* Column sum of a [rows, cols] matrix -> fp32 [cols] (bias gradients). workspace >= hct_colsum_workspace_bytes. */
size_t hct_colsum_workspace_bytes(int rows, int cols);
int hct_colsum(const void* x, int dtype, int rows, int cols, int64_t ld, float* out, void* workspace,
               size_t workspace_bytes, void* stream);

/* dtype conversion / transposed conversion (bf16 working copies of the fp32 master weights).  src_dtype and dst_dtype are
 * HCT_F32 or HCT_BF16, in any of the four pairs; any other code returns HCT_E_BADARG and nothing is written. */
int hct_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);
int hct_transpose_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int rows, int cols, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-parameter gradient clip (src/utils/misc.py:374-383) + AdamW (src/utils/optimizers.py:354-360
 * -> torch.optim.AdamW defaults) over a FLAT fp32 parameter/gradient/state buffer described by a
 * device segment table seg_off[nseg+1] (element offsets; segment i = [seg_off[i], seg_off[i+1])).
 *   hct_grad_norms : norms[i] = ||g_i||_2 ; coef[i] = clip/(norm+1e-6) if < 1 else 1 (clip <= 0: all 1).
 *                    scale_in_place != 0 also multiplies the gradients (the reference's in-place form).
 *   hct_adamw_step : g <- g*coef (written back), decoupled weight decay on every element, bias-corrected
 *                    update; `step` is 1-based; optionally refreshes a bf16 shadow of the parameters.
 *                    skip[i] != 0 freezes segment i (requires_grad = False).
 * Lion / SGD / Lamb (optimizers.py:267-279, torch.optim.SGD as :347-353 builds it, lamb_kernel :154-172) share that contract:
 *   total is a positive multiple of 1024 and every segment starts on a multiple of 1024; coef (may be NULL) is the deferred
 *   per-tensor clip coefficient, and where coef[i] != 1 the clipped gradient g*coef[i] is written back to grads (nothing else
 *   is ever written there); skip (may be NULL): skip[i] != 0 leaves the parameter, every state buffer, the bf16 shadow and, for
 *   Lamb, the three diagnostics of segment i bit for bit as they were; params_bf16 (may be NULL) receives the updated
 *   parameters rounded to bf16 by the kernel that writes params.  Hyper-parameters are doubles (the host derives 1 - beta,
 *   1 - lr*wd in double and rounds once).  No floating-point atomics: the same inputs give the same bits.  No host sync, no
 *   allocation; everything runs on `stream`.
 *   hct_lion_step : p <- p*(1 - lr*wd);  p <- p - lr*sign(beta1*m + (1-beta1)*g)  (m before this step, sign(0) = 0);
 *                   m <- beta2*m + (1-beta2)*g.
 *   hct_sgd_step  : buf <- momentum*buf + g;  p <- p - lr*buf  (no weight decay, dampening 0, no Nesterov).  momentum == 0:
 *                   momentum_buf may be NULL and is not touched, p <- p - lr*g.
 *   hct_lamb_step : m <- beta1*m + (1-beta1)*g;  v <- beta2*v + (1-beta2)*g*g  (no bias correction);
 *                   u = m/(sqrt(v) + eps) + wd*p;  weight_norm[i] = min(||p_i||, 10) of p BEFORE the update;  adam_norm[i] =
 *                   ||u_i||;  trust_ratio[i] = weight_norm/(adam_norm + eps), 1 where either norm is 0;  p <- p - lr*trust_ratio*u.
 *                   Three launches (moments + per-unit partial sums; one block per segment folds them in a fixed order; update
 *                   with u recomputed from the stored moments).  workspace >= hct_lamb_workspace_bytes(total, nseg) bytes
 *                   (8 bytes per 1024 elements), 4-byte aligned.  The first moment is the gradient's, not the squared
 *                   gradient's of the reference's class `Lamb` (optimizers.py:120).
 * ------------------------------------------------------------------------------------------ */
size_t hct_grad_norms_workspace_bytes(int64_t total);
int hct_grad_norms(float* grads, const int64_t* seg_off, int nseg, int64_t total, float clip, int scale_in_place,
                   float* norms, float* coef, void* workspace, size_t workspace_bytes, void* stream);
int hct_adamw_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off,
                   const float* coef, const uint8_t* skip, int nseg, int64_t total, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, void* params_bf16, void* stream);
int hct_lion_step(float* params, float* grads, float* exp_avg, const int64_t* seg_off, const float* coef,
                  const uint8_t* skip, int nseg, int64_t total, double lr, double beta1, double beta2, double weight_decay,
                  void* params_bf16, void* stream);
int hct_sgd_step(float* params, float* grads, float* momentum_buf, const int64_t* seg_off, const float* coef,
                 const uint8_t* skip, int nseg, int64_t total, double lr, double momentum, void* params_bf16, void* stream);
size_t hct_lamb_workspace_bytes(int64_t total, int nseg);
int hct_lamb_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off, const float* coef,
                  const uint8_t* skip, int nseg, int64_t total, double lr, double beta1, double beta2, double eps,
                  double weight_decay, float* weight_norm, float* adam_norm, float* trust_ratio, void* workspace,
                  size_t workspace_bytes, void* params_bf16, void* stream);

/* The same four updates with a per-segment multiplier of the rate and of the decay: the param groups of torch.optim.*
 * (src/utils/optimizers.py:344-379 builds one group; layer-wise rate decay and a no-weight-decay set need one per distinct
 * (lr, weight_decay)) without a launch or a set of state buffers per group.  lr_scale and wd_scale are DEVICE arrays of nseg
 * floats, finite and >= 0; each may be NULL on its own, and NULL means all ones.  Segment s is updated with
 * lr_s = lr*lr_scale[s] and wd_s = weight_decay*wd_scale[s] wherever the update uses lr or weight_decay:
 *   AdamW 1 - lr_s*wd_s and lr_s/(1 - beta1^t);  Lion 1 - lr_s*wd_s and lr_s;  SGD lr_s (it has no decay, hence no wd_scale);
 *   Lamb wd_s inside u in both the moments and the update pass, lr_s*trust_ratio[s] in the update.
 * Everything else is the contract above (1024-aligned segments, deferred clip coefficient applied and written back, skip leaves
 * every bit of a segment, params_bf16 from the kernel that writes params, no atomics, no host sync, same inputs -> same bits).
 * A unit of 1024 elements belongs to one segment, so each block forms its constants in double from the launch scalars and its
 * segment's scales and rounds to float where the host rounds for the unscaled calls: with both arrays all ones (or NULL) the
 * result is bit-equal to the unscaled entry point's.  Cost over the unscaled call: at most two 4-byte loads per block. */
int hct_adamw_step_scaled(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off,
                          const float* coef, const uint8_t* skip, int nseg, int64_t total, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int step, void* params_bf16, const float* lr_scale,
                          const float* wd_scale, void* stream);
int hct_lion_step_scaled(float* params, float* grads, float* exp_avg, const int64_t* seg_off, const float* coef,
                         const uint8_t* skip, int nseg, int64_t total, double lr, double beta1, double beta2, double weight_decay,
                         void* params_bf16, const float* lr_scale, const float* wd_scale, void* stream);
int hct_sgd_step_scaled(float* params, float* grads, float* momentum_buf, const int64_t* seg_off, const float* coef,
                        const uint8_t* skip, int nseg, int64_t total, double lr, double momentum, void* params_bf16,
                        const float* lr_scale, void* stream);
int hct_lamb_step_scaled(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off, const float* coef,
                         const uint8_t* skip, int nseg, int64_t total, double lr, double beta1, double beta2, double eps,
                         double weight_decay, float* weight_norm, float* adam_norm, float* trust_ratio, void* workspace,
                         size_t workspace_bytes, void* params_bf16, const float* lr_scale, const float* wd_scale, void* stream);

/* AdamW with a step count per segment.  torch.optim.AdamW counts updates per parameter: one without a gradient is passed over,
 * and its bias corrections start at 1 with its first gradient (a layer frozen for the first epochs, DINO.FREEZE_LAST_LAYER).
 * hct_adamw_step[_scaled] take one `step` for every segment and are right while every live segment has had the same number of
 * updates; this entry point takes seg_step, a DEVICE array of nseg int32: seg_step[s] >= 1 is the 1-based number of the update
 * this call makes to segment s (the entry of a skipped segment is not read).  Each block forms 1 - beta1^t and 1 - beta2^t of
 * its segment in double and rounds step_size = lr_s/(1 - beta1^t) and 1/sqrt(1 - beta2^t) to float once, as the host does for
 * the other two.  lr_scale / wd_scale as for hct_adamw_step_scaled, each may be NULL.  Everything else is the contract above. */
int hct_adamw_step_counts(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off,
                          const float* coef, const uint8_t* skip, int nseg, int64_t total, float lr, float beta1,
                          float beta2, float eps, float weight_decay, const int32_t* seg_step, void* params_bf16,
                          const float* lr_scale, const float* wd_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whole-model driver (MaskedAutoencoderViT.forward mae.py:303-317 and its autograd backward,
 * engine_pretrain_mae.py:58-62).  The plan is a HOST object describing the parameter layout
 * (names / shapes / offsets into one flat buffer, in the reference's registration order) and the
 * activation workspace layout for a fixed batch size; it owns no device memory.
 * ------------------------------------------------------------------------------------------ */
typedef struct hct_mae_config {
  int input_size, patch_size, in_chans;
  double mask_ratio; /* double: len_keep = (int)(L * (1 - mask_ratio)) must round as the reference's Python float does (mae.py:205) */
  int pos_embed; /* 0 none, 1 learnable, 2 sincos (same storage; init differs on the host) */
  int encoder_depth, encoder_embed_dim, encoder_mlp_dim, encoder_num_heads;
  int decoder_depth, decoder_embed_dim, decoder_mlp_dim, decoder_num_heads;
  int norm_pix_loss, use_bias;
  /* encoder_only = 1 turns the plan into the plain ViT backbone of DINO pre-training (src/models/vit.py:144-173): every patch is
   * embedded (no masking, mask_ratio ignored), class token, num_register_tokens register tokens behind it, encoder blocks, final
   * LayerNorm with final_norm_eps (vit.py:124: 1e-6; 0 = the MAE default 1e-5); no decoder.  Driven by hct_vit_forward /
   * hct_vit_backward_stage instead of hct_mae_forward / hct_mae_backward_stage. */
  int encoder_only, num_register_tokens;
  float final_norm_eps;
  /* LoRA adapters on q and v of every block (attentionblock.py:6-22, 45-47, 57-59; the reference hard-codes 128): 0 = off, otherwise
   * a multiple of 32.  Encoder-only plans only.  Each block then has four more parameters, attn.lora_{q,v}.lora_matrix_{B,A}
   * (B [D, r], A [r, D]); see hct_lora_qv_fwd for what they compute. */
  int lora_rank;
  /* Normalisation layer of every block and of norm / decoder_norm (MAE.NORM_LAYER; mae.py:41, vit.py:51, attentionblock.py:81):
   * 0 = LayerNorm, 1 = RMSNorm (layers.py:11-54).  With 1 the plan has no att_norm.bias / ffn_norm.bias / norm.bias /
   * decoder_norm.bias and every normalisation runs hct_rmsnorm_* with eps 1e-6. */
  int norm_kind;
  /* Dropout rate of the model (MAE.DROPOUT_RATE / VIT.DROPOUT_RATE), 0 <= p < 1: one rate for the five sites of the reference (patch
   * embedding, attention probabilities, proj_drop, MLP drop1 / drop2).  It sizes the extra workspace; whether a forward drops is said
   * per forward by hct_mae_plan_set_dropout. */
  float dropout_rate;
  /* Stochastic depth (VIT.DROP_PATH_RATE), 0 <= r < 1, encoder-only plans only (a plan with a decoder refuses r > 0): block j drops
   * each of its two residual branches per sample at rate q_j = r * j / (encoder_depth - 1) (see "Stochastic depth" above).  Armed per
   * forward by hct_mae_plan_set_dropout, with the same seed as the element masks. */
  float drop_path_rate;
  /* Mask token of the plain ViT (iBOT; encoder-only plans only, a plan with a decoder refuses it): 1 adds the parameter `mask_token`
   * [1, D] behind cls_token / register_tokens and lets the plan run hct_vit_forward_parts_masked.  0 = the layout without it.  The newest
   * field; it sits ahead of patch_dropout so that the double stays the struct's last eight bytes. */
  int mask_token;
  /* Patch dropout (VIT.PATCH_DROPOUT), 0 <= r < 1, encoder-only plans only: the share of patch tokens a forward drops.  With r > 0 the
   * plan keeps K = (int)(L * (1 - r)) patches per volume (evaluated in double, hence a double like mask_ratio; K < 1 is refused), every
   * row count of the encoder follows 1 + R + K, and the plan is driven by hct_vit_forward_parts_keep.  0 = the plan of every patch. */
  double patch_dropout;
} hct_mae_config;

typedef struct hct_mae_plan hct_mae_plan;

typedef struct hct_param_info {
  char name[96];
  int ndim;
  int64_t shape[5];
  int64_t offset; /* element offset into the flat fp32 parameter / gradient buffers */
  int64_t numel;
  int requires_grad;
  int is_matrix;      /* 1: a GEMM weight that gets bf16 (+ transposed bf16) working copies */
  int64_t bf16_t_offset; /* element offset of the transposed bf16 copy in the bf16-T buffer, or -1 */
} hct_param_info;

/* compute_dtype: HCT_F32 (parity mode: every kernel fp32) or HCT_BF16 (bf16 storage + MFMA). */
hct_mae_plan* hct_mae_plan_create(const hct_mae_config* cfg, int batch, int compute_dtype);
void hct_mae_plan_destroy(hct_mae_plan*);
int hct_mae_plan_num_params(const hct_mae_plan*);
int hct_mae_plan_param_info(const hct_mae_plan*, int index, hct_param_info* out);
int64_t hct_mae_plan_param_elems(const hct_mae_plan*);     /* flat fp32 params / grads length (padded) */
int64_t hct_mae_plan_bf16_t_elems(const hct_mae_plan*);    /* transposed-bf16 weight buffer length      */
size_t hct_mae_plan_workspace_bytes(const hct_mae_plan*);  /* activations + scratch                      */
int hct_mae_plan_len_keep(const hct_mae_plan*);            /* visible patches per volume = int(L * (1 - mask_ratio)); encoder-only: L, or int(L * (1 - patch_dropout)) */
/* Compact tail (MAE plans): the loss takes only the masked patches' rows (mae.py:298-299), so with compact != 0 the next
 * forwards run everything behind the last decoder block's attention (its proj / MLP, decoder_norm, decoder_pred, the loss)
 * and the matching backward on those B*(L-K) rows alone.  Loss and every parameter gradient are those of the full
 * computation; the activations "dec<last>.out", "pred_full", "dpred_full" then hold the compact rows (row j of volume b =
 * decoder row tail_rows[b*(L-K)+j], activation "tail_rows") and the kept patches have NO prediction: leave it off (the
 * default) for a forward whose reconstruction of every patch is wanted.  Returns the mode in effect (0 where the geometry
 * does not allow it), < 0 on a null plan.                                                                                */
int hct_mae_plan_set_tail(hct_mae_plan*, int compact);
/* First decoder block on "cat" rows (default on for MAE plans with two or more decoder blocks; HCT_DEC0_TABLE=0 at plan creation or
 * on = 0 here turns it off): the masked tokens enter the decoder as mask_token + pos[l] in every volume (mae.py:259-265), so
 * LayerNorm1 and the qkv Linear of that block run on B*(K+1) kept / class rows + L table rows instead of B*(L+1), forward and
 * backward; same loss, same gradients (the sums over the masked rows are taken per patch position first).  Returns the mode in
 * effect. */
int hct_mae_plan_set_dec0(hct_mae_plan*, int on);
/* Dropout of the next forward (and of its backward): active != 0 on a plan with dropout_rate > 0 draws the masks of `seed` at the
 * sites  0 = patch embedding,  1 + 4 j + {0 attention probabilities, 1 proj_drop, 2 drop1, 3 drop2}  for block j (encoder blocks first,
 * then the decoder's).  While active, proj and linear2 run without their fused residual (a streaming pass adds it), the attention runs
 * the general kernels with the mask, the proj / linear2 bias gradients are column sums of the masked gradient, and the compact tail /
 * first-decoder-block row forms are not used.  With active == 0 or rate 0 the plan issues exactly the launches it issues without
 * dropout.  On a plan with drop_path_rate > 0 the same call arms stochastic depth with the same seed: the forward fills the table of
 * per-sample multipliers (hct_drop_path_scales; its backward reads it again) and every block with q_j > 0 runs its residual adds through
 * hct_residual_drop_apply; a block with q_j = 0 at dropout rate 0 issues exactly the launches it issues without either.  Returns the
 * mode in effect (1 when elements or paths drop), < 0 on a null plan. */
int hct_mae_plan_set_dropout(hct_mae_plan*, int active, uint64_t seed);
/* bind caller-owned device buffers. params_bf16 / params_bf16_t may be NULL in HCT_F32 mode. */
int hct_mae_plan_bind(hct_mae_plan*, float* params, float* grads, void* params_bf16, void* params_bf16_t,
                      void* workspace, size_t workspace_bytes);
/* refresh bf16 + transposed-bf16 working copies from the fp32 master weights (after load / optimizer step).
 * with_plain = 0 skips the plain bf16 copy (hct_adamw_step already wrote it). */
int hct_mae_refresh_weights(hct_mae_plan*, int with_plain, void* stream);
/* forward: x [B,C,S,S,S] of x_dtype (HCT_F32, or HCT_F16 = the persistent cache's storage type, transforms.py:171-178),
 * noise [B,L] fp32 -> *loss (device fp32).  Saves activations in the workspace.
 * grad_scale != 0: training forward -- the loss pass also writes the backward's seed d(loss)/d(pred) * grad_scale (the
 * volume and the prediction are read once per step); grad_scale = 1 / world_size under data parallelism, else 1.
 * grad_scale == 0: inference forward (no backward may follow). */
int hct_mae_forward(hct_mae_plan*, const void* x, int x_dtype, const float* noise, float* loss, float grad_scale, void* stream);
/* device pointer to the scalar dLoss that multiplies the backward's seed (NULL = 1.0; a value of 1.0 costs nothing). */
int hct_mae_set_loss_grad(hct_mae_plan*, const float* dloss);
/* backward in stages so the host can launch the per-bucket gradient all-reduce between them:
 * stage 0 .. hct_mae_num_backward_stages()-1, in order; stage s computes the gradients of the parameter range reported by
 * hct_mae_backward_stage_range (element offsets into the flat buffer; the ranges tile the buffer from its end to its start).
 * In bf16 plans the WEIGHT gradients (dW = dY^T . X, which feed nothing in the backward) of several stages are queued and run
 * together in one grouped launch (hct_gemm_tn_group_*): a range is therefore FINAL only once
 * hct_mae_backward_final_offset() -- every element at or behind it is final -- has moved down to its begin; after the last
 * stage it is 0.  hct_mae_plan_set_wgrad_defer(plan, defer, group_blocks): defer = 0 runs every weight gradient inside its stage
 * (split-K launches, ranges final stage by stage); group_blocks > 0 flushes the queue at least every that many block stages
 * (default 0: once after the decoder's and once after the encoder's backward); returns the mode in effect.  Environment at plan
 * creation: HCT_WGRAD_DEFER=0, HCT_WGRAD_GROUP_BLOCKS=n. */
int hct_mae_num_backward_stages(const hct_mae_plan*);
int hct_mae_backward_stage_range(const hct_mae_plan*, int stage, int64_t* begin, int64_t* end);
int hct_mae_backward_stage(hct_mae_plan*, int stage, void* stream);
int64_t hct_mae_backward_final_offset(const hct_mae_plan*);
int hct_mae_plan_set_wgrad_defer(hct_mae_plan*, int defer, int group_blocks);
/* Frozen parameters.  Every parameter starts with the requires_grad flag hct_mae_plan_param_info reports; flag = 0 marks parameter
 * `index` frozen.  The backward then skips the weight-gradient product of a frozen matrix (a trainable bias keeps its gradient) and
 * does not write the gradient of a frozen cls_token / register_tokens / position table / qkv, patch-embedding, decoder_embed or
 * decoder_pred bias.  This holds for every plan kind and every row form of a block.  Gradients that ride in another kernel's
 * epilogue (LayerNorm weights and biases, the proj / linear1 / linear2 biases) are written whatever their flag says, and so are
 * mask_token and decoder_cls_token when the first decoder block ran on cat rows (hct_mae_plan_set_dec0; on every row a frozen
 * one is skipped): the host zeroes those after the backward.  With every flag at its default the launch sequence is unchanged.
 * hct_mae_refresh_weights(with_plain = 0), the
 * form that follows an optimizer step, also leaves the transposed bf16 copy of a frozen matrix as it is once it has been made. */
int hct_mae_plan_set_requires_grad(hct_mae_plan*, int index, int flag);
/* Plain ViT backbone (plans created with encoder_only = 1).  forward: x [B,C,S,S,S] -> "latent" [B*(1+R+L), D] in the compute
 * dtype = norm(blocks(...)) of every token (hct_mae_plan_activation(plan, "latent")); row b*(1+R+L) is volume b's class token.
 * backward: stages 0 .. hct_mae_num_backward_stages()-1 like the MAE plan (final norm, blocks in reverse, input assembly + patch
 * embedding); stage 0 takes dlatent [B*(1+R+L), D] in the compute dtype (the gradient w.r.t. "latent"; rows that do not
 * feed the loss are zero). */
int hct_vit_forward(hct_mae_plan*, const void* x, int x_dtype, void* stream);
/* The same forward with the batch given as `n_parts` tensors of batch / n_parts volumes each, in batch order: what
 * MultiCropWrapper's torch.cat of equally sized crops (misc.py:467-480) would have produced, without the copy. */
int hct_vit_forward_parts(hct_mae_plan*, const void* const* xs, int n_parts, int x_dtype, void* stream);
int hct_vit_backward_stage(hct_mae_plan*, int stage, const void* dlatent, void* stream);
int hct_vit_assemble_bwd(const float* dh0, int B, int L, int R, int D, void* dtok, int dtok_dtype, float* dcls, float* dreg, float* dpos,
                         void* stream);
/* Patch dropout (hct_mae_config.patch_dropout): the ViT input over the K kept patches of every volume, in shuffle order.
 *   fwd: h0[b,0] = cls;  h0[b,1+r] = reg[r];  h0[b,1+R+j] = tok[b*K+j] + pos[ids_shuffle[b,j]]     h0 [B, 1+R+K, D] fp32
 *   bwd: dtok[b*K+j] = dh0[b,1+R+j];  dcls = sum_b dh0[b,0];  dreg[r] = sum_b dh0[b,1+r];
 *        dpos[l] = sum_{b: l kept} dh0[b, 1+R+ids_restore[b,l]]   (a position no volume kept gets an exact 0)
 * tok / dtok [B*K, D] in their dtype, everything else fp32; ids [B, L] i32 as hct_mask_rank writes them (1 <= K <= L).  reg (R = 0),
 * pos and every gradient may be NULL.  Gradients are written, not accumulated; the sums run in batch order without atomics, so two
 * calls agree bit for bit.  D % 4 == 0. */
int hct_vit_assemble_keep_fwd(const void* tok, int tok_dtype, const float* cls, const float* reg, const float* pos,
                              const int32_t* ids_shuffle, int B, int L, int K, int R, int D, float* h0, void* stream);
int hct_vit_assemble_keep_bwd(const float* dh0, const int32_t* ids_restore, int B, int L, int K, int R, int D, void* dtok, int dtok_dtype,
                              float* dcls, float* dreg, float* dpos, void* stream);
/* The plain ViT forward of a plan created with patch_dropout > 0: noise [B, L] fp32 is ranked (hct_mask_rank: stable, ties to the
 * lower index), volume b keeps the patches ids_shuffle[b, :K] in that order, only those are gathered and embedded, and "latent" is
 * [B*(1+R+K), D].  The ids stay in the plan's "ids_shuffle" / "ids_restore" activations for the backward (hct_vit_backward_stage,
 * unchanged in its calls).  Such a plan refuses hct_vit_forward / hct_vit_forward_parts, and a plan without the rate refuses this. */
int hct_vit_forward_parts_keep(hct_mae_plan*, const void* const* xs, int n_parts, int x_dtype, const float* noise, void* stream);
/* Masked ViT input (iBOT): a masked patch enters the blocks as the learned mask token instead of its embedding.
 *   fwd: h0[b,0] = cls;  h0[b,1+r] = reg[r];  h0[b,1+R+l] = (mask[b,l] ? mask_token : tok[b*L+l]) + pos[l]        h0 [B, 1+R+L, D] fp32
 *   bwd: dtok[b*L+l] = mask[b,l] ? 0 : dh0[b,1+R+l];  dmask_token = sum over the masked (b,l) of dh0[b,1+R+l];
 *        dcls, dreg, dpos as hct_vit_assemble_bwd writes them
 * mask [B, L] uint8 on the device (0 = the patch is seen); tok / dtok [B*L, D] in their dtype, everything else fp32; mask_token [D].
 * reg (R = 0), pos and every gradient may be NULL.  Gradients are written, not accumulated, without atomics: dmask_token is reduced in
 * two fixed-order levels -- block j adds the masked ones of rows 128 j .. 128 j + 127 of the B*L patch rows in row order into
 * partial[j] (workspace), then the partials are added in block order -- so two calls agree bit for bit, and a call without a
 * masked entry writes an exact 0.  D % 4 == 0.  Workspace: hct_vit_assemble_masked_bwd_workspace_bytes (needed for dmask_token only). */
int hct_vit_assemble_masked_fwd(const void* tok, int tok_dtype, const float* cls, const float* reg, const float* pos, const float* mask_token,
                                const uint8_t* mask, int B, int L, int R, int D, float* h0, void* stream);
size_t hct_vit_assemble_masked_bwd_workspace_bytes(int B, int L, int D);
int hct_vit_assemble_masked_bwd(const float* dh0, const uint8_t* mask, int B, int L, int R, int D, void* dtok, int dtok_dtype, float* dcls,
                                float* dreg, float* dpos, float* dmask_token, void* workspace, size_t workspace_bytes, void* stream);
/* The plain ViT forward of a plan created with mask_token = 1, with mask [B, L] uint8 (device) saying which patches enter as the mask
 * token.  The plan copies the mask into an activation of its own, and hct_vit_backward_stage (unchanged in its calls) reads it there.
 * Such a plan also runs hct_vit_forward / hct_vit_forward_parts; the backward of an unmasked forward writes a zero mask_token
 * gradient.  A plan without the flag refuses this call, and so does a plan with patch_dropout > 0 (the kept-patch plan takes no mask). */
int hct_vit_forward_parts_masked(hct_mae_plan*, const void* const* xs, int n_parts, int x_dtype, const uint8_t* mask, void* stream);
/* LoRA adapters of the attention's q and v (csrc/lora.hip).  The reference adds lora(x) [B, N, D] to q [B, H, N, dh] after a RAW
 * reshape: with U = (x1 . A^T) . B^T [N, D] per volume, the dh-wide block r = n' H + h' of U (= U[n', h' dh : (h'+1) dh]) is added
 * to q[head = r / N, token = r % N, :], likewise for v.  x1 [M = B N, D], A [r, D], B [D, r], all of `dtype`; r % 32 == 0.
 *   fwd: T [M, 2r] = x1 . [Aq; Av]^T is written (the backward reads it); U is added in place into the q and v slots of
 *        qkv [B, N, 3, H, dh] (stored value + fp32 accumulator, rounded once).
 *   bwd: dA*, dB* (fp32, overwritten) and dx1 [M, D] += dT . A on top of what the caller put there (the qkv input gradient).
 *        A?T / B?T: optional transposed bf16 copies ([D, r] / [r, D]; NULL = none) that let the bf16 products take the MFMA paths. */
int hct_lora_qv_fwd(const void* x1, const void* Aq, const void* Av, const void* Bq, const void* Bv, int B, int N, int H, int dh, int r, int dtype,
                    void* T, void* qkv, void* stream);
size_t hct_lora_qv_bwd_workspace_bytes(int M, int D, int r, int dtype);
int hct_lora_qv_bwd(const void* dqkv, const void* x1, const void* T, const void* Aq, const void* Av, const void* Bq, const void* Bv,
                    const void* AqT, const void* AvT, const void* BqT, const void* BvT, int B, int N, int H, int dh, int r, int dtype, float* dAq,
                    float* dAv, float* dBq, float* dBv, void* dx1, void* workspace, size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------------------------------
 * Inference with a trained encoder (csrc/retrieval.hip): volume-to-volume retrieval and attention maps (the reference's README;
 * notebooks/extract_feature_sample.ipynb stops at the features).
 *
 * hct_topk_dot: q [Q, D] and g [G, D] are row-major matrices of unit vectors of `dtype` (hct_l2norm_rows_fwd), 16-byte aligned.
 * For every query: the k largest dot products in descending order, equal scores by ascending gallery row; scores [Q, k] fp32,
 * idx [Q, k].  exclude (or NULL): per query one gallery row to skip, -1 = none.  Slots that cannot be filled hold idx -1 and
 * score -inf.  1 <= k <= 64, D % 4 == 0, G < 2^31 (offsets are 64-bit: G * D may exceed 2^31).  The [Q, G] matrix is never
 * formed: the workspace holds the partial lists, Q * chunks * k keys of 8 bytes with chunks = hct_topk_dot_chunks(Q, G) =
 * min(ceil(G / 1024), max(1, 2048 / ceil(Q / 64))).  Deterministic: no atomics, a repeated call is bit-identical, and bitwise-equal
 * gallery rows score bitwise-equal.  bf16 with D % 32 == 0 runs on MFMA, everything else on a plain kernel.
 *
 * hct_attention_row_probs: probs [B, H, n_rows, N] fp32 = softmax_j(q[b, h, rows[r]] . k[b, h, j] dh^-1/2) of the
 * qkv [B, N, 3, H, dh] buffer hct_attention_fwd takes -- the probabilities its single-pass kernels never write.  dh a multiple of
 * 8 up to 128, any N; logits, maximum and sum in fp32.  rows [n_rows] is a DEVICE array of token indices in [0, N): the caller
 * validates it (an index outside the range is read as the nearest valid row, for memory safety only).
 * ------------------------------------------------------------------------------------------ */
int hct_topk_dot_chunks(int Q, int64_t G);
size_t hct_topk_dot_workspace(int Q, int64_t G, int k);
int hct_topk_dot(const void* q, int Q, const void* g, int64_t G, int D, int dtype, const int32_t* exclude, int k, float* scores, int32_t* idx,
                 void* workspace, size_t workspace_bytes, void* stream);
int hct_attention_row_probs(const void* qkv, int B, int N, int H, int dh, int dtype, const int32_t* rows, int n_rows, float* probs, void* stream);
/* ------------------------------------------------------------------------------------------
 * Inference with a trained masked autoencoder (csrc/reconstruct.hip): reconstructions and per-patch error maps accumulated over
 * several masks (headct_foundation_amd/reconstruct.py).
 *
 * hct_mae_recon_accum: pred is the decoder's prediction [B, L (+1 if has_cls_row), pd] (HCT_F32 | HCT_BF16; pd = P^3 C, channel
 * fastest), x [B, C, S, S, S] (HCT_F32 | HCT_F16), mask [B, L] fp32.  A patch with mask == 0 is neither read nor written.  For a
 * masked patch with target t (patchify order): if norm_pix, mu = mean(t), sd = sqrt(var_unbiased(t) + 1e-6), target = (t - mu) / sd,
 * v = pred sd + mu; else target = t, v = pred.  e = mean_k (pred_k - target_k)^2 (the per-patch term of hct_masked_mse's loss).
 * With c = cnt[b, l]: the patch's voxels of recon_sum [B, C, S, S, S] fp32 become (c ? old : 0) + v, err_sum[b, l] becomes
 * (c ? old : 0) + e, cnt[b, l] = c + 1: only cnt [B, L] int32 needs zeroing before the first call.  One writer per element, fixed
 * summation order, no atomics: a repeated sequence of calls is bit-identical.  P % 4 == 0, S % P == 0, pd % 4 == 0; pred, x and
 * recon_sum 16-byte aligned.
 *
 * hct_mae_recon_finish: recon [B, C, S, S, S] fp32 = cnt ? recon_sum / cnt : x (a patch that was never masked shows the scan);
 * err [B, L] fp32 = cnt ? err_sum / cnt : 0; err_vol (or NULL) [B, S, S, S] fp32 = err of the voxel's patch.  recon may be recon_sum.
 * ------------------------------------------------------------------------------------------ */
int hct_mae_recon_accum(const void* pred, int pred_dtype, int has_cls_row, const void* x, int x_dtype /* HCT_F32 | HCT_F16 */, const float* mask,
                        int B, int C, int S, int P, int norm_pix, float* recon_sum, float* err_sum, int32_t* cnt, void* stream);
int hct_mae_recon_finish(const float* recon_sum, const float* err_sum, const int32_t* cnt, const void* x, int x_dtype, int B, int C, int S, int P,
                         float* recon, float* err, float* err_vol, void* stream);
/* ------------------------------------------------------------------------------------------
 * Segmentation fine-tuning (csrc/segmentation.hip; headct_foundation_amd/segmentation.py): an addition of this build.
 *
 * Conventions.  labels are uint8 [B, S, S, S], S = G * P, with values 0 .. K-1; 255 (and any other value >= K) means ignore.
 * logits are the linear decoder's output in TOKEN layout, [rows, K * P^3] of `dtype` (HCT_F32 | HCT_BF16) with row stride ld
 * (elements): column c * P^3 + v is class c at voxel v = (pz * P + py) * P + px of the patch; patch l = (lz * G + ly) * G + lx of
 * sample b is row b * T + first + l and covers z = lz * P + pz (likewise y, x).  first = 1 + registers for the backbone's tokens;
 * first = 0, T = G^3 for bare patch rows.  2 <= K <= 16, B <= 65535, S <= 1024.  With P % 4 == 0, row strides that are multiples
 * of 4 and pointers aligned to 4 elements (labels, pred: 4 bytes; prob: 8 bytes) the kernels move 4 voxels per access; anything
 * else runs one voxel per access with the same arithmetic per voxel.
 *
 * hct_seg_loss: loss = w_ce * CE + w_dice * Dice.  CE = sum_valid w_y nll / sum_valid w_y, nll = -log softmax(x)[y], w =
 * class_weight [K] fp32 (NULL: ones); 0 when no voxel is valid.  Dice is MONAI's DiceLoss(softmax=True, include_background=True,
 * batch=False): per sample b and class c over the valid voxels I = sum p_c [y = c], Pc = sum p_c, Y = sum [y = c],
 * dice_bc = (2 I + 1e-5) / (Pc + Y + 1e-5), Dice = mean_bc (1 - dice_bc); a sample with no valid voxel has dice_bc = 1.
 * Outputs (each may be NULL): loss, ce, dice (one fp32 each), dice_bc [B, K] fp32.  dlogits (or NULL), of the logits' dtype
 * with row stride ldd: d(loss * dloss[0]) / dlogits (dloss NULL: 1), exact zeros at ignored voxels and in the `first` leading rows
 * of every sample; columns past K * P^3 of a row are not touched.  dlogits may be `logits` itself (ldd == ld): the thread that
 * reads a voxel's K logits writes its K gradients.  Softmax in fp32 with the row maximum subtracted; block partials in a fixed
 * order, the final sums in double: no atomics, a repeated call is bit-identical.  reuse_stats != 0 (dlogits given, every loss
 * output NULL): the gradient phase alone, from the workspace as an earlier call with the same logits, labels, shape and weights
 * left it -- forward and backward of a training step then read the logits twice and write them once.
 *
 * hct_seg_predict: per voxel the arg-max class (ties to the lowest class).  pred (or NULL) uint8 [B, S, S, S]; prob (or NULL) fp16
 * [B, S, S, S], the softmax probability of class prob_class; counts (or NULL; needs labels and the workspace) int64 [B, K, 3] =
 * TP, FP, FN per sample and class over the valid voxels, summed in a fixed order.  One pass over the logits.
 *
 * hct_gather_flip_labels: out[b] = flips(pool[slot[b]]), pool uint8 [n_slots, S, S, S], out uint8 [B, S, S, S], flip (or NULL)
 * the per-sample 3-bit code of hct_gather_augment (bit a = spatial axis a).  A slot outside [0, n_slots) -- -1 by contract --
 * gives an all-ignore (255) volume.  S % 4 == 0, both pointers 4-byte aligned.
 *
 * hct_label_to_item: the label twin of the loading chain's last three steps.  ras fp32 [d0, d1, d2] is the mask file after
 * hct_volume_to_ras; out uint8 [R0, R1, R2] takes, by nearest neighbour, the voxel the image's item shows at each position:
 * with box = start[3], size[3] (device int32, the words hct_foreground_bbox left for the IMAGE; confined to the volume here),
 * output index o of axis a lies in resampled cell c = start_a + min(size_a - 1, ((2 o + 1) size_a) / (2 R_a)) (integer
 * division: the cell under the centre of the resize bin), and that cell shows mask voxel near[a][c], near device int32
 * [m0 + m1 + m2], the tables of the three axes one after the other, near[a][j] = clamp(floor(j step_a + 0.5), 0, d_a - 1) with
 * step of headct_foundation_amd.nifti.spacing_geometry.  A value that is no integer in [0, 254] gives 255 and sets status[0]
 * (device int32, zeroed by the call) to HCT_LABEL_BAD_VALUE.  Every axis 1 ... 1024.
 * ------------------------------------------------------------------------------------------ */
size_t hct_seg_loss_workspace_bytes(int B, int G, int P, int K);
int hct_seg_loss(const void* logits, int dtype, int64_t ld, const uint8_t* labels, const float* class_weight, int B, int T, int first, int G,
                 int P, int K, float w_ce, float w_dice, const float* dloss, float* loss, float* ce, float* dice, float* dice_bc,
                 void* dlogits, int64_t ldd, int reuse_stats, void* workspace, size_t workspace_bytes, void* stream);
size_t hct_seg_predict_workspace_bytes(int B, int G, int P, int K);
int hct_seg_predict(const void* logits, int dtype, int64_t ld, const uint8_t* labels, int B, int T, int first, int G, int P, int K,
                    int prob_class, uint8_t* pred, void* prob, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
#define HCT_LABEL_BAD_VALUE 2
int hct_label_to_item(const float* ras, int d0, int d1, int d2, const int32_t* near, int m0, int m1, int m2, const int32_t* box, uint8_t* out,
                      int R0, int R1, int R2, int32_t* status, void* stream);
int hct_gather_flip_labels(const uint8_t* pool, const int32_t* slot, uint8_t* out, int B, int S, int64_t n_slots, const unsigned char* flip,
                           void* stream);
/* ------------------------------------------------------------------------------------------
 * Segmentation on the scan's own grid (csrc/native.hip; headct_foundation_amd/native.py): an addition of this build.
 *
 * hct_seg_to_native: ONE sample's logits in token layout (the conventions above, B = 1: rows first .. first + G^3 - 1 of T, row
 * stride ld, HCT_F32 | HCT_BF16) -> the class of every voxel of the scan's FILE grid, pred int16 [nk, nj, ni] (i contiguous, as
 * read_nifti returns a file).  The geometry comes as four tables over the three file axes, one after the other (i, then j, then
 * k; ni + nj + nk entries each, built on the host in float64 by native.native_tables): file index f of axis a reads item indices
 * i0[f] and i1[f] (int32, used clamped to [0, S - 1]) of item axis o, perm[o] == a, with weight w[f] (fp32) on i1, and lies in the
 * foreground box iff inside[f] (uint8) != 0.  perm0 .. perm2 is nifti.ras_axes' perm, a permutation of 0, 1, 2.  Per voxel: the
 * trilinear blend of the K logits at the 8 taps in fp32 (bf16 widened first; a lerp is a + w * (b - a), first along k, then j,
 * then i), then the arg-max, ties to the lowest class (hct_seg_predict's rule).  A voxel outside on any axis is class 0.
 * class_voxels int64 [K]: voxels per predicted class over the whole grid.  labels (or NULL) uint8 [nk, nj, ni], values >= K
 * (255) = ignore; counts (or NULL; needs labels) int64 [K, 3] = TP, FP, FN over the valid voxels, hct_seg_predict's convention.
 * Integer workgroup partials in the workspace (hct_seg_to_native_workspace_bytes, 4-byte aligned), folded in a fixed order: a
 * repeated call is bit-equal.  2 <= K <= 16, every file axis 1 ... 1024, G * P <= 1024 and K * G * P <= 8192 (two item rows of
 * K * G * P floats are kept in LDS).  Bad arguments return HCT_E_BADARG, too small a workspace HCT_E_WORKSPACE; nothing is
 * launched in either case.  Timed as class 10 of the measurement hooks.
 * ------------------------------------------------------------------------------------------ */
size_t hct_seg_to_native_workspace_bytes(int ni, int nj, int nk, int K);
int hct_seg_to_native(const void* logits, int dtype, int64_t ld, int T, int first, int G, int P, int K, const int32_t* i0, const int32_t* i1,
                      const float* w, const uint8_t* inside, int perm0, int perm1, int perm2, int ni, int nj, int nk, const uint8_t* labels,
                      int16_t* pred, int64_t* class_voxels, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------------------------------
 * Surface-distance metrics on the scan's own grid (csrc/surface.hip; headct_foundation_amd/surface.py): an addition of this build.
 * Volumes are [nk, nj, ni] with i contiguous, every axis 1 ... 32768; a box is [k0, k1) x [j0, j1) x [i0, i1) inside the volume
 * (an empty one launches nothing in hct_edt3d).  Workspaces are 8-byte aligned.  Bad arguments return HCT_E_BADARG, too small a
 * workspace HCT_E_WORKSPACE, and nothing is launched in either case.  No float atomics: a repeated call is bit-equal.
 *
 * hct_surface_edges: pred int16 and labels uint8 of one scan, class cls in [0, 254].  P = (pred == cls and label != 255),
 *   G = (label == cls); a mask voxel is a surface voxel unless its six face neighbours are all mask voxels (a neighbour outside
 *   the volume is background).  flags uint8 [nk, nj, ni], written everywhere: bit 0 = surface of P, bit 1 = surface of G.
 *   out int64 [8] = n_p, n_g, then the box k0, j0, i0, k1, j1, i1 of every flagged voxel (all 0 where there is none).
 * hct_edt3d: for every voxel of the box, the squared distance in float64 to the nearest voxel of the box whose flag byte has a bit
 *   of `bit` (1 ... 255) set, under the spacings (sk, sj, si), finite and > 0: ((dk sk)^2 + (dj sj)^2) + (di si)^2 with every
 *   product and sum rounded once, minimised directly over the candidates in three passes (k, j, i).  +inf where the box holds no
 *   such voxel.  out float64 [nk, nj, ni]; cells outside the box are not touched.  A box longer than 2048 voxels on any axis returns
 *   HCT_E_UNSUPPORTED before any launch.
 * hct_surface_stats: dist_g / dist_p are hct_edt3d's fields of bit 2 / bit 1 over the same box.  counts int64 [4] = n_p, the
 *   number of P's surface voxels with sqrt(dist_g) <= tau, n_g, and the same for G's against dist_p; vals float64 [4] = the sum
 *   and the maximum of sqrt(dist_g) over P's surface voxels, then of sqrt(dist_p) over G's.  Sums in a fixed order (per thread,
 *   a tree over the workgroup, a tree over the workgroups).
 * hct_surface_select: out float64 [4] = sqrt of the squared distances of rank rank_p_lo, rank_p_hi (0-based, ascending, among
 *   dist_g at P's surface voxels) and rank_g_lo, rank_g_hi (dist_p at G's); a rank below 0 gives NaN.  An exact radix select over
 *   the 64-bit patterns, eight passes of eight bits, with integer histograms; ranks must lie below the counts.
 * ------------------------------------------------------------------------------------------ */
size_t hct_surface_edges_workspace_bytes(int nk, int nj, int ni);
int hct_surface_edges(const int16_t* pred, const uint8_t* labels, int nk, int nj, int ni, int cls, uint8_t* flags, int64_t* out, void* workspace,
                      size_t workspace_bytes, void* stream);
int hct_edt3d(const uint8_t* flags, int bit, int nk, int nj, int ni, int k0, int j0, int i0, int k1, int j1, int i1, double sk, double sj, double si,
              double* out, void* stream);
size_t hct_surface_stats_workspace_bytes(int nk, int nj, int ni);
int hct_surface_stats(const uint8_t* flags, const double* dist_g, const double* dist_p, int nk, int nj, int ni, int k0, int j0, int i0, int k1, int j1,
                      int i1, double tau, int64_t* counts, double* vals, void* workspace, size_t workspace_bytes, void* stream);
size_t hct_surface_select_workspace_bytes(void);
int hct_surface_select(const uint8_t* flags, const double* dist_g, const double* dist_p, int nk, int nj, int ni, int k0, int j0, int i0, int k1, int j1,
                       int i1, int64_t rank_p_lo, int64_t rank_p_hi, int64_t rank_g_lo, int64_t rank_g_hi, double* out, void* workspace,
                       size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------------------------------
 * Connected components on the scan's own grid (csrc/components.hip; headct_foundation_amd/components.py): an addition of this build.
 * Volumes are [nk, nj, ni] with i contiguous, every axis 1 ... 32768 and nk * nj * ni <= 2^31 - 2; the linear index of voxel
 * (k, j, i) is v = (k * nj + j) * ni + i, and nvox = nk * nj * ni where a call takes the count alone.  Workspaces are 8-byte
 * aligned.  Bad arguments return HCT_E_BADARG, too small a workspace HCT_E_WORKSPACE, and nothing is launched in either case.
 * Only integer atomics: a repeated call is bit-equal.
 *
 * hct_cc_masks: flags uint8 [nk, nj, ni], written everywhere: bit 0 = P = (pred == cls and label != 255), bit 1 = G = (label == cls),
 *   hct_surface_edges' masks.  labels == NULL: P = (pred == cls) and bit 1 is never set (post-processing, which must not look
 *   at the annotation).  cls in [0, 254].
 * hct_cc_label: the components of the voxels whose flag byte has a bit of `bit` (1 ... 255) set, at connectivity 6, 18 or 26
 *   (face, face + edge, face + edge + corner neighbours; spatial ones: the last voxel of a row is no neighbour of the first of the
 *   next).  label int32 [nk, nj, ni] in ROOT FORM: 0 off the mask, on it 1 + the smallest linear index of the voxel's component.
 *   A lock-free union-find in `label` itself (parent(v) <= v throughout; csrc/components.hip states the argument); this build has
 *   no tile phase, so hct_cc_label_workspace_bytes is 0 and the workspace may be NULL.
 * hct_cc_compact: root form, in place, to the numbers 1 ... n in increasing order of the roots' linear indices (the numbering of
 *   scipy.ndimage.label), by a fixed-order three-level prefix sum over chunks of 4096 voxels; *n_out (device memory) = n.
 * hct_cc_sizes: sizes int64 [n + 1], zeroed by the call: voxels per label (entry 0 stays 0); labels above n are not counted.
 * hct_cc_overlap: overlap int64 [n_a + 1], zeroed by the call: for each label of label_a the number of its voxels whose flag byte
 *   has a bit of bit_b set.
 * hct_cc_remove_small: a voxel with label != 0 and sizes[label] < min_voxels becomes class 0 in pred.
 * hct_cc_count_small: *out (int64, device memory) = how many of the labels 1 ... n have sizes[label] < min_voxels: the components
 *   hct_cc_remove_small removes.  0 <= n <= 2^31 - 2.
 * hct_seg_recount: class_voxels int64 [K] and counts (or NULL; needs labels) int64 [K, 3] = TP, FP, FN over the valid voxels of a
 *   prediction as it stands, with hct_seg_to_native's conventions (a label >= K is ignore; integer workgroup partials in the
 *   workspace, folded in a fixed order).  2 <= K <= 16.
 * hct_cc_tile_dims: host only: the extents of the tile one workgroup labels locally; the axis limit 32768 on every axis in this
 *   build, which has no such phase.
 * ------------------------------------------------------------------------------------------ */
int hct_cc_masks(const int16_t* pred, const uint8_t* labels, int nk, int nj, int ni, int cls, uint8_t* flags, void* stream);
size_t hct_cc_label_workspace_bytes(int nk, int nj, int ni);
int hct_cc_label(const uint8_t* flags, int bit, int nk, int nj, int ni, int connectivity, int32_t* label, void* workspace, size_t workspace_bytes,
                 void* stream);
size_t hct_cc_compact_workspace_bytes(int nk, int nj, int ni);
int hct_cc_compact(int32_t* label, int nk, int nj, int ni, int64_t* n_out, void* workspace, size_t workspace_bytes, void* stream);
int hct_cc_sizes(const int32_t* label, int64_t nvox, int64_t n, int64_t* sizes, void* stream);
int hct_cc_overlap(const int32_t* label_a, int64_t n_a, const uint8_t* flags, int bit_b, int64_t nvox, int64_t* overlap, void* stream);
int hct_cc_remove_small(int16_t* pred, const int32_t* label, const int64_t* sizes, int64_t min_voxels, int64_t nvox, void* stream);
int hct_cc_count_small(const int64_t* sizes, int64_t n, int64_t min_voxels, int64_t* out, void* stream);
size_t hct_seg_recount_workspace_bytes(int nk, int nj, int ni, int K);
int hct_seg_recount(const int16_t* pred, const uint8_t* labels, int nk, int nj, int ni, int K, int64_t* class_voxels, int64_t* counts, void* workspace,
                    size_t workspace_bytes, void* stream);
void hct_cc_tile_dims(int* tk, int* tj, int* ti);
/* named activation lookup for parity tests: returns device pointer + shape/dtype, or NULL. */
const void* hct_mae_plan_activation(const hct_mae_plan*, const char* name, int64_t* rows, int64_t* cols, int* dtype);

/* ------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py roofline leg): when enabled, every launch of a kernel class is bracketed
 * by HIP events on its own stream.  id: 0 GEMM-NT (MFMA), 1 GEMM-TN (MFMA), 2 GEMM-generic,
 * 3 attention fwd, 4 attention bwd, 7 batch assembly out of the device pool (hct_gather_augment; work = voxels),
 * 10 segmentation loss / prediction (hct_seg_loss, hct_seg_predict; work = voxels).
 * hct_prof_read blocks until the recorded launches finished and returns
 * their summed duration, launch count and summed algorithmic work (FLOPs).
 * ------------------------------------------------------------------------------------------ */
void hct_prof_enable(int mask); /* bit i enables kernel class i; 0 = off */
void hct_prof_reset(void);
int hct_prof_read(int id, double* total_ms, int64_t* launches, double* work);
int hct_prof_read_bytes(int id, double* bytes); /* algorithmic bytes (operands read once + outputs written once) of those launches */
/* per-shape view of the same records (GEMM classes): one entry per distinct (M, N, K, epilogue mode, tiles, stream-K tiles) */
typedef struct hct_prof_shape {
  int M, N, K, mode, tiles, sk_tiles;
  int64_t launches;
  double total_ms, work, bytes;
} hct_prof_shape;
int hct_prof_shapes(int id, hct_prof_shape* out, int cap); /* returns the number of distinct keys, -1 on a HIP error */
/* testing hook, attention kernel choice:
 *   0  default (shape-driven: full-row forward up to 544 keys; key-owner backward kernels on the shapes they were tuned for)
 *   1  every call through the fp32-math kernels (the reference, and the only path for fp32)
 *   2  the general MFMA kernels on every shape: online-softmax forward, two-phase backward (the fallbacks of untuned shapes) */
void hct_debug_force_simple_attention(int mode);
/* testing hook, NT GEMM kernel choice (each code sets one option; the others keep their value):
 *   0            auto (default)
 *   128 / 256    force the 128x128 two-stage kernel / the persistent 256x256 kernel
 *   -14 / -15    192-row tiles of the persistent kernel for single-round plain / +residual shapes on (default) / off
 *   -8 / -9      stream-K followers publish a wrong sequence number, so every owner times out (test of the poison path) / off
 *   -20 - w      tile walk of the persistent kernel: w = 0 no bands (default), 1 .. 78 bands of w column tiles, 79 the plan's bands
 *   -100 - n     stream-K only where it saves at least n stage pairs per CU (default 20)
 *   -1000 - k    stream-K only for K >= k (default 512; a huge k switches it off) */
void hct_debug_set_gemm_variant(int v);

#ifdef __cplusplus
}
#endif
#endif /* HEADCT_HIP_H */
