// C ABI for multi-head self-attention (attentionblock.py:54-62).  Dispatch: bf16 storage with a head size the
// MFMA kernels cover -> attention_mfma.hip; everything else (all fp32 parity work) -> attention_simple.hip.
#include "common.h"
#include "philox.h"
#include "prof.h"

namespace hct {
int attention_fwd_simple(const void* qkv, int B, int N, int H, int dh, int dtype, void* o, float* lse, hipStream_t s);
int attention_bwd_simple(const void* qkv, const void* o, const void* d_o, const float* lse, int B, int N, int H, int dh,
                         int dtype, void* dqkv, hipStream_t s);
bool attention_mfma_supported(int N, int H, int dh);
int attention_fwd_mfma(const void* qkv, int B, int N, int H, int dh, void* o, float* lse, hipStream_t s);
int attention_bwd_mfma(const void* qkv, const void* o, const void* d_o, const float* lse, int B, int N, int H, int dh,
                       void* dqkv, hipStream_t s);
int attention_dropout_fwd_simple(const void* qkv, int B, int N, int H, int dh, int dtype, void* o, float* lse, const DropArgs& da, hipStream_t s);
int attention_dropout_bwd_simple(const void* qkv, const void* o, const void* d_o, const float* lse, int B, int N, int H, int dh,
                                 int dtype, void* dqkv, const DropArgs& da, hipStream_t s);
int attention_dropout_fwd_mfma(const void* qkv, int B, int N, int H, int dh, void* o, float* lse, const DropArgs& da, hipStream_t s);
int attention_dropout_bwd_mfma(const void* qkv, const void* o, const void* d_o, const float* lse, int B, int N, int H, int dh, void* dqkv,
                               const DropArgs& da, hipStream_t s);
int check_drop_rate(const char* who, float p);
int g_force_simple_attention = 0;
extern int g_attn_general;
}  // namespace hct

using namespace hct;

extern "C" {

// testing hook: 0 default, 1 the fp32-math kernels of attention_simple.hip, 2 the general MFMA kernels on every shape
void hct_debug_force_simple_attention(int mode) {
  g_force_simple_attention = mode == 1;
  g_attn_general = mode == 2;
}

int hct_attention_fwd(const void* qkv, int B, int N, int H, int dh, int dtype, void* o, float* lse, void* stream) {
  HCT_REQUIRE(B > 0 && N > 0 && H > 0 && dh > 0, "hct_attention_fwd: bad shape");
  ProfScope ps(PROF_ATTN_FWD, 4.0 * B * H * (double)N * N * dh, (hipStream_t)stream);
  if (dtype == HCT_BF16 && !g_force_simple_attention && attention_mfma_supported(N, H, dh))
    return attention_fwd_mfma(qkv, B, N, H, dh, o, lse, (hipStream_t)stream);
  return attention_fwd_simple(qkv, B, N, H, dh, dtype, o, lse, (hipStream_t)stream);
}

int hct_attention_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, int B, int N, int H, int dh,
                      int dtype, void* dqkv, void* stream) {
  HCT_REQUIRE(B > 0 && N > 0 && H > 0 && dh > 0, "hct_attention_bwd: bad shape");
  ProfScope ps(PROF_ATTN_BWD, 10.0 * B * H * (double)N * N * dh, (hipStream_t)stream);
  if (dtype == HCT_BF16 && !g_force_simple_attention && attention_mfma_supported(N, H, dh))
    return attention_bwd_mfma(qkv, o, d_o, lse, B, N, H, dh, dqkv, (hipStream_t)stream);
  return attention_bwd_simple(qkv, o, d_o, lse, B, N, H, dh, dtype, dqkv, (hipStream_t)stream);
}

// Attention with dropout on the probabilities (attentionblock.py:61, SDPA(dropout_p = p) in training): O = (softmax(S) o Z) V with the
// counter-based keep mask Z of (seed, site) -- hct_dropout_mask kind 1 -- scaled by 1 / (1 - p).  Same dispatch rule as the plain pair:
// bf16 storage at a head size the MFMA kernels cover -> the general MFMA pair with the mask, everything else the fp32-math kernels.
int hct_attention_dropout_fwd(const void* qkv, int B, int N, int H, int dh, int dtype, float p, uint64_t seed, int site, void* o, float* lse,
                              void* stream) {
  HCT_REQUIRE(B > 0 && N > 0 && H > 0 && dh > 0 && site >= 0, "hct_attention_dropout_fwd: bad shape or site");
  if (int rc = check_drop_rate("hct_attention_dropout_fwd", p)) return rc;
  const DropArgs da = make_drop_args(seed, site, p);
  ProfScope ps(PROF_ATTN_FWD, 4.0 * B * H * (double)N * N * dh, (hipStream_t)stream);
  if (dtype == HCT_BF16 && !g_force_simple_attention && attention_mfma_supported(N, H, dh))
    return attention_dropout_fwd_mfma(qkv, B, N, H, dh, o, lse, da, (hipStream_t)stream);
  return attention_dropout_fwd_simple(qkv, B, N, H, dh, dtype, o, lse, da, (hipStream_t)stream);
}

int hct_attention_dropout_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, int B, int N, int H, int dh, int dtype, float p,
                              uint64_t seed, int site, void* dqkv, void* stream) {
  HCT_REQUIRE(B > 0 && N > 0 && H > 0 && dh > 0 && site >= 0, "hct_attention_dropout_bwd: bad shape or site");
  if (int rc = check_drop_rate("hct_attention_dropout_bwd", p)) return rc;
  const DropArgs da = make_drop_args(seed, site, p);
  ProfScope ps(PROF_ATTN_BWD, 10.0 * B * H * (double)N * N * dh, (hipStream_t)stream);
  if (dtype == HCT_BF16 && !g_force_simple_attention && attention_mfma_supported(N, H, dh))
    return attention_dropout_bwd_mfma(qkv, o, d_o, lse, B, N, H, dh, dqkv, da, (hipStream_t)stream);
  return attention_dropout_bwd_simple(qkv, o, d_o, lse, B, N, H, dh, dtype, dqkv, da, (hipStream_t)stream);
}

}  // extern "C"
