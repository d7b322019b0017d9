// Counter-based dropout masks ("Dropout"): Philox4x32-10 keyed by the 64-bit seed.  A mask is a pure function of
// (seed, site, element), never stored: every kernel that needs one -- forward, backward, hct_dropout_mask -- draws it again.
#pragma once
#include <stdint.h>

namespace hct {

// what a kernel needs to draw keep decisions: key, site, threshold T = floor(p 2^32) and the kept values' scale 1 / (1 - p)
struct DropArgs {
  uint32_t seed_lo, seed_hi, site, thresh;
  float scale;
};

struct Philox4 { uint32_t w[4]; };

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// streaming sites: the four words of elements 4 * group .. 4 * group + 3 of the row-major tensor the site acts on
__host__ __device__ __forceinline__ Philox4 drop_words_stream(const DropArgs& a, uint64_t group) {
  return philox4x32_10((uint32_t)group, (uint32_t)(group >> 32), 0u, a.site, a.seed_lo, a.seed_hi);
}
// attention site: the four words of keys 4 * kgroup .. 4 * kgroup + 3 of query q in (batch, head) bh
__host__ __device__ __forceinline__ Philox4 drop_words_attn(const DropArgs& a, uint32_t kgroup, uint32_t q, uint32_t bh) {
  return philox4x32_10(kgroup, q, bh, a.site, a.seed_lo, a.seed_hi);
}
// multiplier of one element: 1 / (1 - p) where its word keeps it, else 0
__host__ __device__ __forceinline__ float drop_mul(const DropArgs& a, uint32_t word) { return word >= a.thresh ? a.scale : 0.f; }

// host side: arguments of rate p (0 <= p < 1, as fp32) -- T from the fp32 value of p, scale in fp32
inline DropArgs make_drop_args(uint64_t seed, int site, float p) {
  DropArgs a;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
  a.site = (uint32_t)site;
  a.thresh = (uint32_t)((double)p * 4294967296.0);
  a.scale = 1.0f / (1.0f - p);
  return a;
}

}  // namespace hct
